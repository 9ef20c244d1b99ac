"""B3 leaf filter, B2 de-skew and B9 re-framing on the GPU held to the independent reference (tests/pre_reference.py), route by route.  -m gpu.

Leaf filter: every case asserts (a) bit-equality with the reference, shapes included, and (b) the route the filter took, from the product's own read-out
(rgc_voxelgrid_route) -- on a fresh context, as the second and third cloud on a context that holds a kept box, with host and device pointers, and through
rgc_voxelgrid_begin / _end.  The inputs and the restated rule that sized them are in tests/pre_cases.py (checked without a GPU by
tests/test_pre_reference.py); here the read-out is the judge.
De-skew / re-framing: at most one fp32 ulp at the reference's value plus 8 * 2^-53 * (|p| + |t|) (pre_reference.ulp_bound); the largest difference seen
is printed per test."""
import ctypes as C

import numpy as np
import pytest

import pre_cases as pc
import pre_reference as pr

pytestmark = pytest.mark.gpu

ERR_GRID_TOO_LARGE, ERR_NONFINITE = -4, -6


class Ctx:
    """one context through the C-ABI: the filter with host pointers, device pointers and in two halves, and its read-out"""

    def __init__(self):
        from rgc_slam_amd import _lib
        self.m, self.L = _lib, _lib.load()
        h = C.c_void_p()
        assert self.L.rgc_create(0, None, C.byref(h)) == 0
        self.h = h
        self.bufs = []

    def close(self):
        for p in self.bufs:
            self.L.rgc_device_free(self.h, C.c_void_p(p))
        self.L.rgc_destroy(self.h)

    def route(self):
        r = self.m.VgRoute()
        assert self.L.rgc_voxelgrid_route(self.h, C.byref(r)) == 0
        return {k: (list(getattr(r, k)) if k in ("minb", "div") else int(getattr(r, k))) for k, _ in self.m.VgRoute._fields_}

    def dev(self, nbytes):
        p = C.c_void_p()
        assert self.L.rgc_device_alloc(self.h, max(nbytes, 16), C.byref(p)) == 0
        self.bufs.append(p.value)
        return p.value

    def up(self, a):
        a = np.ascontiguousarray(a, np.float32)
        d = self.dev(a.nbytes)
        assert self.L.rgc_upload(self.h, C.c_void_p(d), a.ctypes.data, a.nbytes) == 0
        return d

    def down(self, d, n):
        out = np.empty((n, 4), np.float32)
        if n:
            assert self.L.rgc_download(self.h, out.ctypes.data, C.c_void_p(d), out.nbytes) == 0
        return out

    def host(self, a, leaf):
        """-> (status, output)"""
        a = np.ascontiguousarray(a, np.float32)
        out = np.full((a.shape[0], 4), -77.0, np.float32)
        n = C.c_int(-1)
        rc = self.L.rgc_voxelgrid(self.h, a.ctypes.data, a.shape[0], a.strides[0], C.c_float(leaf), out.ctypes.data, C.byref(n), 0)
        return rc, out[:max(n.value, 0)].copy()

    def device(self, a, leaf):
        a = np.ascontiguousarray(a, np.float32)
        d_in, d_out = self.up(a), self.dev(16 * len(a))
        n = C.c_int(-1)
        rc = self.L.rgc_voxelgrid(self.h, C.c_void_p(d_in), a.shape[0], a.strides[0], C.c_float(leaf), C.c_void_p(d_out), C.byref(n), 1)
        return rc, self.down(d_out, max(n.value, 0))

    def begin(self, a, leaf):
        a = np.ascontiguousarray(a, np.float32)
        d_in, d_out = self.up(a), self.dev(16 * len(a))
        return self.L.rgc_voxelgrid_begin(self.h, C.c_void_p(d_in), a.shape[0], a.strides[0], C.c_float(leaf), C.c_void_p(d_out)), d_out

    def end(self, d_out):
        n = C.c_int(-1)
        rc = self.L.rgc_voxelgrid_end(self.h, C.byref(n))
        return rc, self.down(d_out, max(n.value, 0))


@pytest.fixture
def ctx():
    c = Ctx()
    yield c
    c.close()


_REF = {}


def ref_of(key, cloud, leaf):
    """the reference of a cloud, computed once per module"""
    k = (key, len(cloud), float(leaf))
    if k not in _REF:
        _REF[k] = pr.voxelgrid(cloud, leaf)
    return _REF[k]


def same(got, ref, what):
    rc, out = got
    assert rc == 0, (what, rc)
    ok = out.shape == ref.out.shape and np.array_equal(out.view(np.uint32), ref.out.view(np.uint32))
    assert ok, "%s: %s" % (what, pr.explain_mismatch(ref, out))


def route_label(r):
    if r["path"] == 3:
        return "copy"
    assert r["chain"] == 1, r
    return pc.label(dict(kind="chain", leaf_buckets=r["leaf_buckets"], seg_shift=r["seg_shift"], packed=r["packed"]))


@pytest.mark.parametrize("name", list(pc.route_cases()))
def test_route(name, capsys):
    """one row of the route table: fresh context (host pointers); then, on a context whose kept box comes from ANOTHER cloud of the same volume, as second
    and third cloud on that kept box (host pointers, device pointers) and through begin / end with a blocking filter of the same leaf size in between.
    Bit-equal to the reference every time; the route from the read-out every time.  (Clouds that LEAVE the kept box: test_box_eviction_drift_and_jump.)"""
    cs = pc.route_cases()[name]
    leaf = cs["leaf"]
    fresh, kept = cs["make"](cs["n_fresh"]), cs["make"](cs["n_kept"])
    rf, rk = ref_of(name, fresh, leaf), ref_of(name, kept, leaf)
    seen = []
    c = Ctx()
    try:
        assert c.route()["path"] == 0
        same(c.host(fresh, leaf), rf, "fresh")
        r = c.route(); seen.append(("fresh", r))
        assert (r["path"], r["repeated"], r["kept_box"], r["status"], r["n"], r["n_out"]) == (2, 0, 0, 0, len(fresh), len(rf.out)), r
        assert route_label(r) == cs["want"], r
        assert r["minb"] == list(rf.minb) and r["div"] == list(rf.div) and r["edge"] == 0 and r["flags"] == 0, (r, rf.minb, rf.div)
    finally:
        c.close()
    c = Ctx()
    try:
        same(c.host(cs["make"](cs["n_kept"] - 1), leaf), ref_of(name, cs["make"](cs["n_kept"] - 1), leaf), "the cloud the kept box comes from")
        b0 = c.route()
        assert b0["path"] == 2
        same(c.device(fresh, leaf), rf, "second cloud")
        r = c.route(); seen.append(("second", r))
        assert (r["path"], r["repeated"], r["kept_box"], r["kept_flags"] & 3) == (1, 0, 1, 0), r
        for how in ("host", "device"):
            same(getattr(c, how)(kept, leaf), rk, "third cloud, " + how)
            r = c.route(); seen.append(("kept " + how, r))
            assert (r["path"], r["repeated"], r["kept_box"], r["kept_flags"] & 3, r["flags"] & 3) == (1, 0, 1, 0, 0), r
            assert route_label(r) == cs["want_kept"] and r["edge"] in (4, 16), r
            pad = 32 if not r["leaf_buckets"] else 8
            assert r["div"] == [d + 2 * pad for d in b0["div"]] and r["minb"] == [m - pad for m in b0["minb"]], (r, b0)
        rc, d_out = c.begin(kept, leaf)
        assert rc == 0
        before = c.route()
        assert before == seen[-1][1]                             # begin alone does not change the read-out
        same(c.device(fresh, leaf), rf, "blocking filter of the same leaf size between begin and end")
        same(c.end(d_out), rk, "begin / end")
        r = c.route(); seen.append(("begin/end", r))
        assert (r["path"], r["repeated"], r["kept_box"], r["flags"] & 3, r["n"], r["n_out"]) == (1, 0, 1, 0, len(kept), len(rk.out)), r
        assert route_label(r) == cs["want_kept"], r
        if cs.get("fullest_over"):
            assert pc.fullest_row(fresh, leaf) > 4095 and pc.fullest_row(kept, leaf) > 4095
        if cs.get("wide_x"):
            assert all(x[1]["div"][0] > 8192 and x[1]["seg_shift"] == 13 and x[1]["packed"] == 1 for x in seen if x[0] != "second")
    finally:
        c.close()
    with capsys.disabled():
        for tag, r in seen:
            print("\n  %-18s %-12s path=%d %s seg_shift=%d nseg=%d packed=%d grid=%s" % (name, tag, r["path"], route_label(r), r["seg_shift"], r["nseg"], r["packed"], r["div"]), end="")


@pytest.mark.parametrize("pop", [4095, 4096, 4097])
def test_bucket_population_at_the_packed_field_limit(ctx, pop):
    """whole rows, packed records: the fullest bucket holds exactly 4095 (the last population the 12-bit field holds), 4096 and 4097 points"""
    c = pc.exact_bucket(pop)
    assert pc.fullest_row(c, 0.2) == pop
    ref = ref_of("bucket%d" % pop, c, 0.2)
    for how in ("host", "device", "host"):
        same(getattr(ctx, how)(c, 0.2), ref, "bucket of %d, %s" % (pop, how))
        r = ctx.route()
        assert route_label(r) == "rows packed", r


def test_dense_cloud_on_a_kept_sparse_box_and_back(ctx):
    """a context that holds a sweep's box: a 450 k-point cloud inside it is dense for that box (leaf buckets on the kept box), the sweep after it is sparse again"""
    sw = pc.sweep()
    dense = pc.box_cloud(450000, [-30, -30, -1.5], [30, 30, 4], 19)
    same(ctx.host(sw, 0.2), ref_of("sw", sw, 0.2), "sweep")
    box = ctx.route()
    assert (np.abs(dense[:, :3]).max(axis=0) < np.abs(sw[:, :3]).max(axis=0)).all()
    same(ctx.host(dense, 0.2), ref_of("dense450k", dense, 0.2), "dense on the sweep's box")
    r = ctx.route()
    assert (r["path"], r["leaf_buckets"], r["seg_shift"], r["kept_flags"] & 2) == (1, 1, 0, 0), r
    assert r["div"] == [d + 16 for d in box["div"]], (r, box)
    dropped = r["box_invalidated"]                               # (the dense cloud's floor may lie within 4 leaves of the dense box's: flag 4)
    assert dropped == (1 if r["kept_flags"] & 4 else 0)
    same(ctx.host(sw[5:], 0.2), ref_of("sw5", sw[5:], 0.2), "sweep again")
    r = ctx.route()
    assert r["leaf_buckets"] == 0 and r["path"] == (2 if dropped else 1), r
    same(ctx.host(sw, 0.2), ref_of("sw", sw, 0.2), "and again")
    r = ctx.route()
    assert r["leaf_buckets"] == 0 and r["path"] == 1, r


def test_unfiltered_copy_and_the_grids_just_below(ctx):
    """more than INT_MAX leaves: output = input (RGC_VG_PATH_UNFILTERED), at 12-, 16- and 32-byte strides, the intensity column 0 for a 12-byte point.
    Just below: a sparse grid is filtered; a grid under INT_MAX leaves with more than 64e6 rows is REFUSED (RGC_ERR_GRID_TOO_LARGE) where PCL filters --
    the documented limit of the product."""
    over = pc.two_clusters(4000, 160.0, 31)
    for st in (12, 16, 32):
        a = pc.strided(over, st)
        ref = pr.voxelgrid(a, 0.1)
        assert ref.unfiltered
        for how in ("host", "device"):
            same(getattr(ctx, how)(a, 0.1), ref, "unfiltered, stride %d, %s" % (st, how))
            r = ctx.route()
            assert (r["path"], r["chain"], r["n_out"], r["div"]) == (3, 0, 4000, list(ref.div)), r
    rc, d_out = ctx.begin(over, 0.1)
    same((rc, np.zeros((4000, 4), np.float32)) if rc else ctx.end(d_out), pr.voxelgrid(over, 0.1), "unfiltered through begin / end")
    assert ctx.route()["path"] == 3
    under = pc.two_clusters(4000, 60.0, 31)
    same(ctx.host(under, 0.1), pr.voxelgrid(under, 0.1), "sparse grid under INT_MAX")
    assert ctx.route()["chain"] == 1 and ctx.route()["leaf_buckets"] == 0
    refused = pc.two_clusters(4000, (0.0, 8050.0, 8050.0), 31, span=(20.0, 40.0, 40.0))
    ref = pr.voxelgrid(refused, 1.0)
    assert not ref.unfiltered and float(ref.div[1]) * ref.div[2] > 64e6
    rc, out = ctx.host(refused, 1.0)
    r = ctx.route()
    assert rc == ERR_GRID_TOO_LARGE and len(out) == 0 and (r["status"], r["path"], r["chain"], r["div"]) == (ERR_GRID_TOO_LARGE, 2, 0, list(ref.div)), (rc, r)
    same(ctx.host(under, 0.1), pr.voxelgrid(under, 0.1), "after the refusal")


def test_leaf_sizes_and_walls(ctx):
    """leaf sizes beyond the five in use (and a few drawn from a fixed seed), points on leaf walls and their fp32 neighbours either side, near the origin
    and 500 - 1000 m out; each twice, so that the second run is on the kept box"""
    sw = pc.sweep(n_az=600)
    for leaf in pc.LEAVES_BEYOND + pc.drawn_leaves() + pc.LEAVES_IN_USE:
        walls = pc.wall_points(leaf, 41)
        for k in range(2):
            same(ctx.host(sw, leaf), ref_of("sw600", sw, leaf), "sweep leaf %g run %d" % (leaf, k))
            same(ctx.host(walls, leaf), ref_of("walls", walls, leaf), "walls leaf %g run %d" % (leaf, k))
    c2 = Ctx()
    try:
        for leaf in (0.05, 0.1, 0.15, 0.25):
            for far in (500.0, 1000.0):
                w = pc.wall_points(leaf, 42, far=far)
                for k in range(2):
                    same(c2.host(w, leaf), ref_of("walls%g" % far, w, leaf), "walls at %g m leaf %g run %d" % (far, leaf, k))
                assert c2.route()["path"] == 1
    finally:
        c2.close()


def test_cloud_sizes_and_strides(ctx):
    """n either side of the 64-, 256-, 2048- and 4096-slot boundaries of the chain's kernels: all points in one leaf, every point its own leaf, runs of 3;
    strides of 12, 16, 20, 32 and 4096 bytes (the padding holds a value no output may show)"""
    for n in pc.SIZES:
        for kind, c in pc.sized_clouds(n, 43).items():
            ref = ref_of(kind, c, 0.2)
            for how in ("host", "device"):
                same(getattr(ctx, how)(c, 0.2), ref, "%s n=%d %s" % (kind, n, how))
    sw = pc.sweep(n_az=300)
    for st in pc.STRIDES:
        a = pc.strided(sw, st)
        ref = pr.voxelgrid(a, 0.3)
        for how in ("host", "device"):
            same(getattr(ctx, how)(a, 0.3), ref, "stride %d %s" % (st, how))
        rc, d_out = ctx.begin(a, 0.3)
        assert rc == 0
        same(ctx.end(d_out), ref, "stride %d begin / end" % st)
        if st == 12:
            assert not ref.out[:, 3].any()


def test_box_eviction_drift_and_jump(ctx):
    """the context keeps four boxes round-robin: five, then six leaf sizes in turn, then the first again (its box was evicted: measured); a cloud that
    drifts until flag 4 fires (filtered, the box dropped for the next call), the call after it (measured), and a jump out of the box (repeated)"""
    sw = pc.sweep(n_az=600)
    leaves = (0.2, 0.3, 0.15, 0.4, 0.7, 1.1)
    for leaf in leaves[:4]:
        same(ctx.host(sw, leaf), ref_of("sw600", sw, leaf), "leaf %g" % leaf)
        assert ctx.route()["path"] == 2
    for leaf in leaves[:4]:
        same(ctx.host(sw, leaf), ref_of("sw600", sw, leaf), "leaf %g again" % leaf)
        assert ctx.route()["path"] == 1, "four boxes are kept"
    same(ctx.host(sw, leaves[4]), ref_of("sw600", sw, leaves[4]), "fifth")         # evicts 0.2's box
    assert (ctx.route()["path"], ctx.route()["kept_box"]) == (2, 0)
    same(ctx.host(sw, leaves[1]), ref_of("sw600", sw, leaves[1]), "0.3 survives the fifth")
    assert ctx.route()["path"] == 1
    same(ctx.host(sw, leaves[5]), ref_of("sw600", sw, leaves[5]), "sixth")         # evicts 0.3's
    same(ctx.host(sw, leaves[0]), ref_of("sw600", sw, leaves[0]), "the first again")
    r = ctx.route()
    assert (r["path"], r["kept_box"], r["repeated"]) == (2, 0, 0), r
    same(ctx.host(sw, leaves[0]), ref_of("sw600", sw, leaves[0]), "the first, kept again")
    assert ctx.route()["path"] == 1
    # drift: 0.2 m leaves, padding 32, edge 16 -- a shift of 22 leaves stays inside and comes within 16 leaves of a face
    drift = sw.copy(); drift[:, 0] += np.float32(4.5)
    same(ctx.host(drift, 0.2), ref_of("drift", drift, 0.2), "drifted")
    r = ctx.route()
    assert (r["path"], r["kept_flags"], r["box_invalidated"], r["repeated"]) == (1, 4, 1, 0), r
    same(ctx.host(drift, 0.2), ref_of("drift", drift, 0.2), "the call after flag 4")
    r = ctx.route()
    assert (r["path"], r["kept_box"], r["repeated"]) == (2, 3, 0), r
    jump = sw.copy(); jump[:, :3] += np.float32([60.0, -35.0, 8.0])
    same(ctx.host(jump, 0.2), ref_of("jump", jump, 0.2), "jumped out")
    r = ctx.route()
    assert (r["path"], r["repeated"], r["kept_flags"] & 2, r["box_invalidated"]) == (2, 1, 2, 1), r
    rc, d_out = ctx.begin(sw, 0.2)                                                  # back: outside the jumped box, end repeats it
    assert rc == 0
    same(ctx.end(d_out), ref_of("sw600", sw, 0.2), "begin / end out of the box")
    r = ctx.route()
    assert (r["path"], r["repeated"], r["kept_box"], r["kept_flags"] & 2) == (2, 1, 1, 2), r


def test_kept_box_that_no_longer_fits(ctx):
    """a kept box whose PADDED grid is over INT_MAX leaves while the cloud's own box is under it: the kept box is not used (kept_box = 2), the cloud is
    measured and filtered"""
    a = pc.two_clusters(4000, (115.0, 115.0, 115.0), 33, span=(10.0, 10.0, 10.0))    # 1250^3 = 1.95e9 leaves of 0.1 m; padded by 64: 1314^3 > INT_MAX
    ref = pr.voxelgrid(a, 0.1)
    assert not ref.unfiltered and np.prod([float(d) + 64 for d in ref.div]) > 2147483647.0 and np.prod([float(d) + 16 for d in ref.div]) > (1 << 29)
    same(ctx.host(a, 0.1), ref, "first")
    assert ctx.route()["path"] == 2
    same(ctx.host(a, 0.1), ref, "second")
    r = ctx.route()
    assert (r["path"], r["kept_box"], r["repeated"]) == (2, 2 if np.prod([float(d) for d in ref.div]) <= 2.0e9 else 3, 0), r


@pytest.mark.parametrize("name", ["rows_packed", "leaf_buckets", "segments_300k", "rows_unpacked", "segments_unpacked", "seg13_wide"])
def test_nonfinite_is_refused_on_every_route(ctx, name):
    """NaN / inf / 1e30 in a cloud: RGC_ERR_NONFINITE from the measured box and from the kept one, and the next finite cloud on the context bit-equal again"""
    cs = pc.route_cases()[name]
    leaf, good = cs["leaf"], cs["make"](cs["n_kept"])
    ref = ref_of(name, good, leaf)
    for k, v in enumerate((np.nan, np.inf, -np.inf, 1e30)):
        bad = good.copy(); bad[len(bad) // 2 + k, k % 3] = v
        rc, _ = ctx.host(bad, leaf)
        assert rc == ERR_NONFINITE and ctx.route()["status"] == ERR_NONFINITE, (k, v, rc, ctx.route())
        same(ctx.host(good, leaf), ref, "after %r" % v)
    assert ctx.route()["path"] == 1 and route_label(ctx.route()) == cs["want_kept"], ctx.route()
    bad = good.copy(); bad[7, 1] = np.nan
    rc, d_out = ctx.begin(bad, leaf)
    assert rc == 0
    rc, _ = ctx.end(d_out)
    assert rc == ERR_NONFINITE
    same(ctx.device(good, leaf), ref, "after a NaN through begin / end")


# ---- de-skew and re-framing ------------------------------------------------------------------------------------------------------------
def _within(got, ref, p, t, what):
    bound = pr.ulp_bound(ref, np.linalg.norm(p[:, :3].astype(np.float64), axis=1), np.full(len(p), np.linalg.norm(t)))
    err = np.abs(got[:, :3].astype(np.float64) - ref).astype(np.float64)
    w, k = pr.worst_in_ulps(got[:, :3], ref)
    assert (err <= bound).all(), "%s: %.3f ulp at point %d (%s), got %s reference %s" % (what, w, k // 3, p[k // 3], got[k // 3, :3], ref[k // 3].astype(np.float64))
    return w


def _deskew(ctx, a, q, t, on_device):
    a = np.array(a, np.float32, order="C", copy=True)
    q, t = np.ascontiguousarray(q, np.float64), np.ascontiguousarray(t, np.float64)
    dp = C.POINTER(C.c_double)
    if on_device:
        d = ctx.up(a)
        assert ctx.L.rgc_deskew(ctx.h, C.c_void_p(d), a.shape[0], a.strides[0], q.ctypes.data_as(dp), t.ctypes.data_as(dp), 1) == 0
        assert ctx.L.rgc_download(ctx.h, a.ctypes.data, C.c_void_p(d), a.nbytes) == 0
    else:
        assert ctx.L.rgc_deskew(ctx.h, a.ctypes.data, a.shape[0], a.strides[0], q.ctypes.data_as(dp), t.ctypes.data_as(dp), 0) == 0
    return a


def _transform(ctx, a, q, t, on_device):
    a = np.ascontiguousarray(a, np.float32)
    q, t = np.ascontiguousarray(q, np.float64), np.ascontiguousarray(t, np.float64)
    dp = C.POINTER(C.c_double)
    out = np.full((a.shape[0], 4), -77.0, np.float32)
    if on_device:
        d, d_out = ctx.up(a), ctx.dev(out.nbytes)
        assert ctx.L.rgc_transform_cloud(ctx.h, C.c_void_p(d), a.shape[0], a.strides[0], q.ctypes.data_as(dp), t.ctypes.data_as(dp), C.c_void_p(d_out), 1) == 0
        return ctx.down(d_out, len(a))
    assert ctx.L.rgc_transform_cloud(ctx.h, a.ctypes.data, a.shape[0], a.strides[0], q.ctypes.data_as(dp), t.ctypes.data_as(dp), out.ctypes.data, 0) == 0
    return out


def test_deskew_every_slerp_branch(ctx, capsys):
    """w < 0 (q and -q: the same cloud, bit for bit), identity, w either side of the 1 - eps switch, rotations up to 3.1 rad about tilted axes, a quaternion
    off unit norm; intensities with fraction 0, 0.05, 0.0999 and rings up to 127; translations of 0.3 m and 300 m; points at 1 m and 1 km; host and
    device pointers; strides 16, 20, 32, 4096"""
    worst = 0.0
    for scale in (1.0, 1000.0):
        cloud = pc.deskew_cloud(scale, 51)
        for t in pc.TRANSLATIONS:
            outs = {}
            for name, q in pc.deskew_quats().items():
                ref = pr.deskew(cloud, q, t)
                got = _deskew(ctx, cloud, q, t, False)
                worst = max(worst, _within(got, ref, cloud, t, "deskew %s |p|~%g t=%s" % (name, scale, t)))
                assert np.array_equal(got[:, 3], cloud[:, 3])
                assert np.array_equal(_deskew(ctx, cloud, q, t, True), got), name
                outs[name] = got
            for name in outs:
                if "-(" + name + ")" in outs:
                    assert np.array_equal(outs[name], outs["-(" + name + ")"]), "q and -q differ: " + name
    cloud, q, t = pc.deskew_cloud(30.0, 52, n=777), pc.deskew_quats()["-(small)"], pc.TRANSLATIONS[0]
    ref = pr.deskew(cloud, q, t)
    for st in (16, 20, 32, 4096):
        a = pc.strided(cloud, st)
        for dev in (False, True):
            got = _deskew(ctx, a, q, t, dev)
            _within(got, ref, cloud, t, "deskew stride %d" % st)
            assert np.array_equal(got[:, 3:], a[:, 3:])                          # intensity and padding untouched
    with capsys.disabled():
        print("\n  de-skew: worst %.3f fp32 ulp" % worst, end="")


def test_transform_cloud_against_the_reference(ctx, capsys):
    """re-framing with the de-skew test's quaternions and random unit ones, |t| up to 1e4 m, points at 1 m, 1 km and 10 km; strides 12 .. 4096"""
    worst = 0.0
    rng = np.random.default_rng(61)
    quats = list(pc.deskew_quats().values()) + list(pc.random_unit_quats(12, 62))
    for scale in (1.0, 1000.0, 1.0e4):
        cloud = pc.deskew_cloud(scale, 63)
        for q in quats:
            for tn in (0.3, 300.0, 1.0e4):
                t = rng.normal(size=3); t *= tn / np.linalg.norm(t)
                ref = pr.transform(cloud, q, t)
                got = _transform(ctx, cloud, q, t, False)
                worst = max(worst, _within(got, ref, cloud, t, "transform |p|~%g q=%s t=%s" % (scale, q, t)))
                assert np.array_equal(got[:, 3], cloud[:, 3])
    cloud, q, t = pc.deskew_cloud(30.0, 64, n=777), quats[-1], np.array([300.0, -20.0, 5.0])
    ref = pr.transform(cloud, q, t)
    for st in pc.STRIDES:
        a = pc.strided(cloud, st)
        for dev in (False, True):
            got = _transform(ctx, a, q, t, dev)
            _within(got, ref, cloud, t, "transform stride %d" % st)
            assert np.array_equal(got[:, 3], cloud[:, 3] if st > 12 else np.zeros(len(cloud), np.float32))
    with capsys.disabled():
        print("\n  re-framing: worst %.3f fp32 ulp" % worst, end="")
