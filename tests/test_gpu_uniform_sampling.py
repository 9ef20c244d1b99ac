"""rgc_uniform_sampling on the GPU held to the independent reference (tests/us_reference.py), route by route.  -m gpu.
Every comparison is exact: the winners' points as uint32 views, their input indices, the shapes.  Every case asserts the route the chain took from the
product's own read-out (rgc_voxelgrid_route), and its census minima are those of tests/us_cases.py (checked without a GPU by tests/test_us_reference.py)."""
import ctypes as C

import numpy as np
import pytest

import pre_cases as pc
import pre_reference as pr
import us_cases as uc
import us_reference as us
from test_gpu_pre_routes import Ctx, route_label

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_GRID_TOO_LARGE, ERR_NONFINITE = -1, -4, -6


class UsCtx(Ctx):
    def us_host(self, a, leaf, index=True):
        """-> (status, points, indices)"""
        a = np.ascontiguousarray(a, np.float32)
        out, idx = np.full((a.shape[0], 4), -77.0, np.float32), np.full(a.shape[0], -5, np.int32)
        n = C.c_int(-1)
        rc = self.L.rgc_uniform_sampling(self.h, a.ctypes.data, a.shape[0], a.strides[0], C.c_float(leaf), out.ctypes.data, idx.ctypes.data if index else None,
                                         C.byref(n), 0)
        m = max(n.value, 0)
        assert (idx[m:] == -5).all() and (index or (idx == -5).all())
        return rc, out[:m].copy(), idx[:m].copy() if index else None

    def us_device(self, a, leaf, index=True):
        a = np.ascontiguousarray(a, np.float32)
        d_in, d_out, d_idx = self.up(a), self.dev(16 * len(a)), self.dev(4 * len(a))
        n = C.c_int(-1)
        rc = self.L.rgc_uniform_sampling(self.h, C.c_void_p(d_in), a.shape[0], a.strides[0], C.c_float(leaf), C.c_void_p(d_out), C.c_void_p(d_idx) if index else None,
                                         C.byref(n), 1)
        m = max(n.value, 0)
        idx = np.empty(m, np.int32)
        if m and index:
            assert self.L.rgc_download(self.h, idx.ctypes.data, C.c_void_p(d_idx), idx.nbytes) == 0
        return rc, self.down(d_out, m), idx if index else None


@pytest.fixture
def ctx():
    c = UsCtx()
    yield c
    c.close()


_REF = {}


def ref_of(key, cloud, leaf):
    k = (key, len(cloud), float(leaf))
    if k not in _REF:
        _REF[k] = us.uniform_sampling(cloud, leaf)
    return _REF[k]


def same(got, ref, what):
    rc, out, idx = got
    assert rc == 0, (what, rc)
    assert out.shape == ref.out.shape, "%s: %s outputs, reference %s" % (what, out.shape, ref.out.shape)
    if idx is not None:
        bad = np.flatnonzero(idx != ref.index)
        assert len(bad) == 0, "%s: %d of %d winners differ; first: output %d got point %d reference %d (leaf of %d members)" % (
            what, len(bad), len(idx), bad[0], idx[bad[0]], ref.index[bad[0]], 0 if ref.unfiltered else len(ref.leaf.members(bad[0])))
    assert np.array_equal(out.view(np.uint32), ref.out.view(np.uint32)), what


def test_lattice_exact_ties(ctx):
    """coordinates k / 16 at leaf 0.5: exact ties for the minimum in >= 20 leaves, the winner not the leaf's first member in >= 100; host and device pointers,
    with and without out_index, a 12-byte stride (c = 0), negative coordinates"""
    c = uc.lattice()
    ref = ref_of("lattice", c, 0.5)
    cen = ref.census()
    for k, v in uc.LATTICE_MINIMA.items():
        assert cen[k] >= v, cen
    labels = []
    for how in ("us_host", "us_device"):
        for index in (True, False):
            same(getattr(ctx, how)(c, 0.5, index), ref, "lattice %s index=%s" % (how, index))
            r = ctx.route()
            assert (r["n"], r["n_out"], r["status"], r["path"]) == (len(c), len(ref.index), 0, 1 if labels else 2), r
            labels.append(route_label(r))
    # measured: 24 x 24 x 8 leaves for 3000 points, dense; then the kept box padded by 32 leaves a side, sparse for them
    assert labels == ["leaf buckets", "rows packed", "rows packed", "rows packed"], labels
    xyz = np.ascontiguousarray(c[:, :3])
    assert xyz.strides[0] == 12
    r3 = ref_of("lattice3", xyz, 0.5)
    assert not r3.out[:, 3].any() and np.array_equal(r3.index, ref.index)
    for how in ("us_host", "us_device"):
        same(getattr(ctx, how)(xyz, 0.5), r3, "12-byte stride " + how)


@pytest.mark.parametrize("spread", [False, True], ids=["leaf_buckets", "rows"])
@pytest.mark.parametrize("plant", ["first", "last", "boundary"])
def test_leaf_populations_at_every_kernel_boundary(ctx, plant, spread):
    """leaves of 1, 2, 63 / 64 / 65, 255 / 256 / 257, 2047 / 2048 / 2049, 4095 / 4096 / 4097 and 6000 points; the winner planted as the first member, the last,
    and just below the boundary slot with an exact copy just above it; dense grid (leaf buckets) and sparse grid (whole rows, the fullest over the packed
    record's population field); the second run is on the kept box"""
    c, planted = uc.big_leaves(plant, spread=spread)
    ref = ref_of("big %s %s" % (plant, spread), c, 0.5)
    assert set(int(x) for x in planted) <= set(int(x) for x in ref.index) and ref.leaf.fullest == 6000
    want = "rows packed" if spread else "leaf buckets"
    for k, how in enumerate(("us_host", "us_device")):
        same(getattr(ctx, how)(c, 0.5), ref, "%s %s run %d" % (plant, want, k))
        r = ctx.route()
        assert route_label(r) == want and r["path"] == (2, 1)[k], r
    if spread:
        assert pc.fullest_row(c, 0.5) > 4095


@pytest.mark.parametrize("leaf", [0.3, 0.2])
def test_points_on_leaf_walls(ctx, leaf):
    c = uc.walls(leaf)
    assert uc.rounding_decides(c, leaf) >= 10
    ref = ref_of("walls", c, leaf)
    for k in range(2):
        same(ctx.us_host(c, leaf), ref, "walls leaf %g run %d" % (leaf, k))
        assert ctx.route()["chain"] == 1 and ctx.route()["path"] == (2, 1)[k]


@pytest.mark.parametrize("name", ["rows_packed", "sweep_0.2", "leaf_buckets", "segments_300k", "bucket_over_4095", "rows_unpacked", "segments_unpacked", "seg13_wide"])
def test_every_route_of_the_chain(name):
    """the leaf filter's route table (tests/pre_cases.py) through UniformSampling: measured box on a fresh context, then the kept box (host and device
    pointers); seg13_wide is a grid more than 8192 leaves wide"""
    cs = pc.route_cases()[name]
    leaf = cs["leaf"]
    fresh, kept = cs["make"](cs["n_fresh"]), cs["make"](cs["n_kept"])
    rf, rk = ref_of(name, fresh, leaf), ref_of(name, kept, leaf)
    c = UsCtx()
    try:
        same(c.us_host(fresh, leaf), rf, "fresh")
        r = c.route()
        assert (r["path"], r["repeated"], r["kept_box"], r["status"], r["n"], r["n_out"]) == (2, 0, 0, 0, len(fresh), len(rf.index)), r
        assert route_label(r) == cs["want"] and r["minb"] == list(rf.leaf.minb) and r["div"] == list(rf.leaf.div), r
        if cs.get("wide_x"):
            assert r["div"][0] > 8192 and r["seg_shift"] == 13
    finally:
        c.close()
    c = UsCtx()
    try:
        first = cs["make"](cs["n_kept"] - 1)
        same(c.us_host(first, leaf), ref_of(name, first, leaf), "the cloud the kept box comes from")
        for how in ("us_host", "us_device"):
            same(getattr(c, how)(kept, leaf), rk, "kept box, " + how)
            r = c.route()
            assert (r["path"], r["repeated"], r["kept_box"], r["kept_flags"] & 3) == (1, 0, 1, 0) and route_label(r) == cs["want_kept"], r
    finally:
        c.close()


@pytest.mark.parametrize("n_half,want", [(2500, "seg13 packed"), (1500, "segments unpacked")])
def test_wide_grid_with_members_to_choose_from(ctx, n_half, want):
    """a grid more than 8192 leaves wide (2 km at 0.1 m) whose leaves hold two points: every point of the corridor and a copy moved by about a sixth of a
    leaf, so that about a third of the winners are not their leaf's first member; seg_shift = 13 with packed records, and unpacked records"""
    c = pc.far_x(n_half, 16)
    c = np.concatenate([c, c + np.float32([0.013, 0.007, 0.011, 1.0])])
    c = np.ascontiguousarray(c[np.random.default_rng(1).permutation(len(c))])
    ref = ref_of("wide", c, 0.1)
    assert ref.leaf.div[0] > 8192 and ref.census()["winner_not_first"] >= 100 and ref.census()["fullest"] >= 2
    for k, how in enumerate(("us_host", "us_device")):
        same(getattr(ctx, how)(c, 0.1), ref, "wide run %d" % k)
        r = ctx.route()
        assert r["div"][0] > 8192 and r["chain"] == 1 and r["path"] == (2, 1)[k], r
        if k == 0:                                                   # (the padded kept box of the second run has more rows: its buckets may differ)
            assert route_label(r) == want and (want != "seg13 packed" or r["seg_shift"] == 13), r


def test_kept_box_left_and_repeated(ctx):
    """a cloud that jumps out of the kept box: the chain runs on the kept box, sees a point outside, and the sampling is repeated on the measured box"""
    sw = pc.sweep(n_az=600)
    same(ctx.us_host(sw, 0.2), ref_of("sw600", sw, 0.2), "sweep")
    same(ctx.us_host(sw, 0.2), ref_of("sw600", sw, 0.2), "sweep, kept")
    assert ctx.route()["path"] == 1
    jump = sw.copy(); jump[:, :3] += np.float32([60.0, -35.0, 8.0])
    same(ctx.us_device(jump, 0.2), ref_of("jump", jump, 0.2), "jumped out")
    r = ctx.route()
    assert (r["path"], r["repeated"], r["kept_flags"] & 2, r["box_invalidated"]) == (2, 1, 2, 1), r
    same(ctx.us_host(jump, 0.2), ref_of("jump", jump, 0.2), "and kept again")
    assert ctx.route()["path"] == 1


def test_refusals_next_to_good_calls(ctx):
    """the unfiltered copy (identity indices, the input's bits), RGC_ERR_GRID_TOO_LARGE, RGC_ERR_NONFINITE, bad arguments, n = 0 -- each followed by a call that
    must be right"""
    good = uc.lattice()
    rg = ref_of("lattice", good, 0.5)
    over = pc.two_clusters(4000, 160.0, 31)
    over[5, 0] = np.float32(-0.0)                                         # the copy keeps bits
    for st in (12, 16, 32):
        a = pc.strided(over, st)
        ref = us.uniform_sampling(a, 0.1)
        assert ref.unfiltered and np.array_equal(ref.index, np.arange(4000))
        for how in ("us_host", "us_device"):
            same(getattr(ctx, how)(a, 0.1), ref, "unfiltered, stride %d, %s" % (st, how))
            r = ctx.route()
            assert (r["path"], r["chain"], r["n_out"], r["div"]) == (3, 0, 4000, list(ref.leaf.div)), r
        same(ctx.us_host(good, 0.5), rg, "after the copy")
    refused = pc.two_clusters(4000, (0.0, 8050.0, 8050.0), 31, span=(20.0, 40.0, 40.0))
    rc, out, idx = ctx.us_host(refused, 1.0)
    r = ctx.route()
    assert rc == ERR_GRID_TOO_LARGE and len(out) == 0 and (r["status"], r["path"], r["chain"]) == (ERR_GRID_TOO_LARGE, 2, 0), (rc, r)
    same(ctx.us_host(good, 0.5), rg, "after the refusal")
    for k, v in enumerate((np.nan, np.inf, -np.inf, 1e30)):
        bad = good.copy(); bad[len(bad) // 2 + k, k % 3] = v
        for how in ("us_host", "us_device"):
            rc, out, idx = getattr(ctx, how)(bad, 0.5)
            assert rc == ERR_NONFINITE and len(out) == 0 and ctx.route()["status"] == ERR_NONFINITE, (v, rc)
            same(getattr(ctx, how)(good, 0.5), rg, "after %r" % v)
    rc, out, idx = ctx.us_host(good[:0], 0.5)
    assert rc == 0 and len(out) == 0 and ctx.route()["path"] == 0
    n = C.c_int(-1)
    o = np.zeros((len(good), 4), np.float32)
    for leaf, stride in ((0.0, 16), (-1.0, 16), (np.nan, 16), (np.inf, 16), (0.5, 8), (0.5, 18)):
        assert ctx.L.rgc_uniform_sampling(ctx.h, good.ctypes.data, len(good), stride, C.c_float(leaf), o.ctypes.data, None, C.byref(n), 0) == ERR_INVALID
    same(ctx.us_host(good, 0.5), rg, "after the bad arguments")


def test_leaf_filter_on_the_same_context_is_undisturbed(ctx):
    """rgc_voxelgrid before and after rgc_uniform_sampling on one context returns what it returns alone (bit for bit the reference's), on the kept box too"""
    sw = pc.sweep(n_az=600)
    vg, ur = pr.voxelgrid(sw, 0.2), ref_of("sw600", sw, 0.2)
    alone = UsCtx()
    try:
        rc, first = alone.host(sw, 0.2)
        rc2, second = alone.host(sw, 0.2)
        assert rc == 0 and rc2 == 0
    finally:
        alone.close()
    assert np.array_equal(first.view(np.uint32), vg.out.view(np.uint32)) and np.array_equal(first.view(np.uint32), second.view(np.uint32))
    for k in range(2):
        rc, out = ctx.host(sw, 0.2)
        assert rc == 0 and np.array_equal(out.view(np.uint32), first.view(np.uint32)), k
        same(ctx.us_host(sw, 0.2), ur, "sampling between two filters")
        same(ctx.us_device(sw, 0.2), ur, "sampling between two filters, device")
    rc, out = ctx.device(sw, 0.2)
    assert rc == 0 and np.array_equal(out.view(np.uint32), first.view(np.uint32)) and ctx.route()["path"] == 1


def test_python_layer(ctx):
    from rgc_slam_amd import registration
    c = uc.lattice()
    ref = ref_of("lattice", c, 0.5)
    out, idx = registration.uniform_sampling(c, 0.5, return_index=True)
    assert np.array_equal(idx, ref.index) and np.array_equal(out.view(np.uint32), ref.out.view(np.uint32))
    assert np.array_equal(registration.uniform_sampling(c, 0.5).view(np.uint32), ref.out.view(np.uint32))
