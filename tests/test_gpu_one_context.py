"""Every subsystem interleaved on ONE rgc_ctx, against the same calls on contexts of their own (rgc::OdometryNode, odometry.Preprocessor and the owner=
parameter of the Python classes all put several subsystems on one context: one stream, one source-preparation stream, the pinned staging, d_small /
h_small, the leaf filter's scratch, the box hints, the profiling state, solve_in_flight -- and every DevBuf may be reallocated by ensure() next to another
subsystem's kept state).  The operations, their inputs and what each leaves on a context are tests/one_context_ops.py's table.

Every comparison is of BYTES (one_context_ops.diff): the header promises run-to-run and host / device identity for all of these.  No tolerance in this file."""
import ctypes as C
import threading

import numpy as np
import pytest

import one_context_ops as oc

pytestmark = pytest.mark.gpu

NAMES = sorted(oc.OPS)


@pytest.fixture(scope="module")
def lone():
    """lone results: each operation on a fresh context of its own, computed once per (operation, size, form) and shared (one_context_ops.lone caches them)"""
    oc.P()
    return oc.lone


@pytest.fixture()
def ctx():
    c = oc.Ctx()
    yield c
    if c.vg_open is not None:                    # (a failed test may leave the filter open: its buffers go with the context)
        c.vg_open = None
    c.close()


def _first(name):
    return oc.OPS[name].forms[0]


# ---- every ordered pair -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a", NAMES)
def test_every_ordered_pair(lone, ctx, a):
    """A, then for every B: B (= lone B), what A left is unchanged unless the header says B replaces it (one_context_ops.drops), A again (= lone A).  An
    operation that can be left open (the leaf filter's halves) is begun before B and ended behind it."""
    A = oc.OPS[a]
    fa = _first(a)
    oc.check(ctx, a, "small", fa)
    kept_a = A.kept(ctx)
    for i, b in enumerate(n for n in NAMES if n != a):
        B = oc.OPS[b]
        if A.begin:
            ctx.history.append("%s: begin" % a)
            A.begin(ctx, A.make("small"))
        oc.check(ctx, b, "small", B.forms[i % len(B.forms)])
        if A.begin:
            ctx.history.append("%s: end" % a)
            bad = oc.diff(A.end(ctx), lone(a, "small", fa))
            assert not bad, "%s left open across %s differs at %s\nhistory: %s" % (a, b, ", ".join(bad[:8]), " -> ".join(ctx.history))
        if not oc.drops(b, a):
            oc.check_kept(ctx, a, kept_a, b)
        oc.check(ctx, a, "small", fa, what="A again, after %s" % b)
        oc.check_kept(ctx, a, kept_a, "%s and %s again" % (b, a))


# ---- buffers that grow under kept state -----------------------------------------------------------------------------------------------------------------------
def test_buffers_that_grow_under_kept_state(lone, ctx):
    """every operation at small, then at large (every ensure() reallocates), then at small again; each result equals lone, and after each round every kept
    record that no later operation of the round replaced equals what it was right after its own operation"""
    n = 0
    for k, size in enumerate(("small", "large", "small")):
        n += oc.run_schedule(ctx, [(name, size, oc.OPS[name].forms[(k + i) % len(oc.OPS[name].forms)], 0, False) for i, name in enumerate(NAMES)])
    assert n >= 3 * len(NAMES)


# ---- device hand-offs in stream order ----------------------------------------------------------------------------------------------------------------------------
class View:
    """device memory that a stage left behind, as the next stage's input (quacks like keyframes.DeviceCloud); nothing is synchronised"""

    def __init__(self, c, ptr, n, stride=16):
        self._h, self._L, self.ptr, self.n, self.stride_bytes, self._c = c.h, c.L, ptr, int(n), stride, c

    def __len__(self):
        return self.n

    @property
    def addr(self):
        return self.ptr.value if isinstance(self.ptr, C.c_void_p) else int(self.ptr)

    def synchronize(self):
        raise AssertionError("a stage on the same context must not need a synchronisation")

    def numpy(self, cols=4, dtype=np.float32):
        out = np.empty((self.n, cols), dtype)
        if out.nbytes:
            self._c.chk(self._L.rgc_download(self._h, out.ctypes.data, self.ptr, out.nbytes))
        return out


def _alone(fn):
    c = oc.Ctx()
    try:
        return fn(c)
    finally:
        c.close()


def _same(got, want, stage, c):
    bad = oc.diff(got, want)
    assert not bad, "stage '%s' of the chain differs from the same stage on a context of its own, run from the host copy of its input, at %s\nhistory: %s" % (
        stage, ", ".join(bad[:8]), " -> ".join(c.history))


def _sor_raw(c, src, n, on_device, out, idx):
    kept = C.c_int(0)
    c.chk(c.L.rgc_outlier_statistical(c.h, src, n, 16, on_device, 8, 1.0, 0, out, idx, None, C.byref(kept)))
    return kept.value


def _normals_raw(c, src, n, on_device, out):
    prm = oc.P()._lib.NormalParams()
    prm.k, prm.flip, prm.radius = 10, 1, 0.0
    valid = C.c_int(0)
    c.chk(c.L.rgc_normal_estimate(c.h, src, n, 16, None, 0, 0, on_device, C.byref(prm), out, None, None, None, C.byref(valid)))
    return valid.value


def _features_at_the_end(c, cloud, normals):
    """FPFH with given normals, clustering and plane on one cloud (host arrays or Views), through the Python classes on context c"""
    f = c.view("fpfh"); f._init_params(); f.setInputCloud(cloud); f.setInputNormals(normals); f.setRadiusSearch(1.0)
    out = dict(fpfh=f.compute(), fpfh_counts=f.getCounts())
    e = c.view("cluster"); e.setInputCloud(cloud); e.setClusterTolerance(0.6); e.setMinClusterSize(3); e.setMaxClusterSize(2 ** 31 - 1)
    e.extract()
    out.update(labels=e.labels(), offsets=e.offsets())
    s = c.view("plane"); s._init_params(); s.setInputCloud(cloud); s.setDistanceThreshold(0.1); s.setMaxIterations(30); s.setSeed(3)
    idx, coeff = s.segment()
    out.update(plane_idx=idx, plane_coeff=coeff)
    return out


def _chain_3(c, sweep):
    """rgc_transform_cloud on the device -> rgc_set_source_device (prepared on its own stream) -> normals of the same buffer, on the shared context behind
    chain 2's scan and solve.  one_context_ops.route() puts the scan grid's cell size AND its kept box back first: behind another sweep's box 15 more
    far-field points of this one go to the cooperative kernel (rgc_stats::deferred_source 2054 against 2039) and 4 of its 5729 covariances differ by one
    ulp from a lone context's -- with the cell size alone put back this stage failed"""
    L = c.L
    c.history.append("chain 3")
    reg, v, xyzi = oc.reg_inputs("small"), c.view("vgicp"), sweep["xyzi"]
    q, t = np.array([0.0, 0.0, np.sin(0.01), np.cos(0.01)]), np.array([0.05, -0.02, 0.0])
    oc.route(c)
    d_in, d_tf, d_tgt = oc.Dev(c, xyzi), oc.Dev(c, np.zeros_like(xyzi)), oc.Dev(c, reg["tgt"])
    v.transformCloudDevice(d_in.addr, len(xyzi), 16, q, t, d_tf.addr)          # enqueued before rgc_set_target*: the source may be handed over unsynchronised
    v.setInputTargetDevice(d_tgt.addr, len(d_tgt), d_tgt.stride_bytes)
    v.setInputSourceDevice(d_tf.addr, len(xyzi), 16)
    ne = c.view("normal"); ne._init_params(); ne.setInputCloud(View(c, d_tf.ptr, len(xyzi))); ne.setKSearch(8)
    nrm = ne.compute()
    src_cov = v.getSourceCovariances()
    eye = np.eye(4, dtype=np.float32)
    fp = C.POINTER(C.c_float)
    held = np.empty((len(xyzi), 3), np.float32)
    c.chk(L.rgc_get_aligned(c.h, eye.ctypes.data_as(fp), held.ctypes.data_as(fp), 12))
    h_tf = d_tf.numpy()
    _same(h_tf, _alone(lambda a: a.view("pre").transformPointCloud(xyzi, q, t)), "rgc_transform_cloud on the device", c)

    def source_alone(a):
        oc.route(a)
        a.v.setInputTarget(reg["tgt"]); a.v.setInputSource(h_tf)
        out = np.empty((len(h_tf), 3), np.float32)
        a.chk(a.L.rgc_get_aligned(a.h, eye.ctypes.data_as(fp), out.ctypes.data_as(fp), 12))
        return [out, a.v.getSourceCovariances()]
    _same([held, src_cov], _alone(source_alone), "rgc_set_source_device on the re-framed buffer (the points it holds, its covariances)", c)
    _same(nrm, _alone(lambda a: a.view("pre").normalEstimation(h_tf, k=8)), "normals of the buffer the source preparation reads", c)
    c.hold("reg", [d_in, d_tf, d_tgt])


def test_device_hand_offs_in_stream_order(lone, ctx):
    clouds = []                                  # the store's device clouds: freed through the context, so closed while it is alive whatever happens
    try:
        _chains(ctx, clouds)
    finally:
        for icp_end in ("_src", "_tgt"):
            setattr(ctx.view("icp"), icp_end, None)
        for dc in clouds:
            dc.close()


def _chains(ctx, clouds):
    c, L = ctx, ctx.L
    sweep, other = oc.scan_inputs("small", 400, 5100), oc.us_inputs("small")["xyzc"]
    # chain 1: front-end cloud on the device -> leaf filter begun; uniform sampling of another cloud while it is open; ended -> SOR -> normals -> FPFH, clustering, plane
    c.history.append("chain 1")
    fe = c.view("fe").laserCloudHandler(sweep["raw"], diagnostics=False, cloud=False)
    dc, n = C.c_void_p(), C.c_int(0)
    c.chk(L.rgc_frontend_cloud_device(c.h, C.byref(dc), C.byref(n)))
    n = n.value
    assert n == fe["n_cloud"] > 1000
    d_vg = oc.Dev(c, np.zeros((n, 4), np.float32))
    c.chk(L.rgc_voxelgrid_begin(c.h, dc, n, 16, C.c_float(0.4), d_vg.ptr))
    d_other, d_us, d_usi = oc.Dev(c, other), oc.Dev(c, np.zeros_like(other)), oc.Dev(c, np.zeros(len(other), np.int32), np.int32)
    n_us = C.c_int(0)
    c.chk(L.rgc_uniform_sampling(c.h, d_other.ptr, len(other), 16, C.c_float(0.5), d_us.ptr, d_usi.ptr, C.byref(n_us), 1))
    n_vg = C.c_int(0)
    c.chk(L.rgc_voxelgrid_end(c.h, C.byref(n_vg)))
    n_vg = n_vg.value
    d_sor, d_sidx = oc.Dev(c, np.zeros((n_vg, 4), np.float32)), oc.Dev(c, np.zeros(n_vg, np.int32), np.int32)
    n_sor = _sor_raw(c, d_vg.ptr, n_vg, 1, d_sor.ptr, d_sidx.ptr)
    d_nrm = oc.Dev(c, np.zeros((n_sor, 4), np.float32))
    n_valid = _normals_raw(c, d_sor.ptr, n_sor, 1, d_nrm.ptr)
    end = _features_at_the_end(c, View(c, d_sor.ptr, n_sor), View(c, d_nrm.ptr, n_sor))
    # the host copies, downloaded only now, and every stage alone from the host copy of its input
    h_cloud = View(c, dc, n).numpy()
    h_vg, h_us, h_usi = d_vg.numpy()[:n_vg], d_us.numpy()[:n_us.value], d_usi.numpy()[:n_us.value]
    h_sor, h_sidx, h_nrm = d_sor.numpy()[:n_sor], d_sidx.numpy()[:n_sor], d_nrm.numpy()
    _same(h_cloud, _alone(lambda a: a.view("fe").laserCloudHandler(sweep["raw"], diagnostics=False)["cloud"]), "front-end cloud left on the device", c)
    _same(h_vg, _alone(lambda a: a.view("pre").voxelGridFilter(h_cloud, 0.4)), "leaf filter in halves on the front-end's device cloud", c)
    _same([h_us, h_usi], list(_alone(lambda a: a.view("pre").uniformSampling(other, 0.5, return_index=True))), "uniform sampling while the leaf filter is open", c)
    _same([h_sor, h_sidx], list(_alone(lambda a: a.view("pre").statisticalOutlierRemoval(h_vg, 8, 1.0, return_index=True))), "SOR on the leaf filter's device output", c)
    def normals_alone(a):
        out = np.empty((n_sor, 4), np.float32)
        return [out, _normals_raw(a, h_sor.ctypes.data, n_sor, 0, out.ctypes.data)]
    h_sor = np.ascontiguousarray(h_sor)
    _same([h_nrm, n_valid], _alone(normals_alone), "normals on SOR's device output", c)
    _same(end, _alone(lambda a: _features_at_the_end(a, h_sor, h_nrm)), "FPFH with the device normals, clustering and plane on the same buffer", c)
    for d in (d_vg, d_other, d_us, d_usi, d_sor, d_sidx, d_nrm):
        d.free()

    # chain 2: rgc_kf_assemble(on_device) -> search index, NDT target, VGICP target + align, ICP on two assembled clouds
    c.history.append("chain 2")
    drive, reg = oc.drive_inputs("large"), oc.reg_inputs("small")
    store = oc._kf_fill(c, drive)
    dc_map = store.assemble(drive["ids"][:8], (2,), leaf=0.3, device=True)
    clouds.append(dc_map)
    dc_scan = store.assemble(drive["ids"][8:10], (1,), leaf=0.0, device=True)
    clouds.append(dc_scan)
    qry = np.ascontiguousarray(drive["clouds"][3][1][:500, :3])
    tree = c.view("tree"); tree.setInputCloud(dc_map)
    knn = list(tree.nearestKSearch(qry, 8))
    p = oc.P()
    ndt = c.view("ndt"); ndt.setResolution(1.0); ndt.setDistanceMode(p.ndt.NDT_D2D); ndt.setNeighborSearchMethod(p.ndt.NDT_DIRECT7)
    ndt.setInputTarget(dc_map); ndt.setInputSource(dc_scan)
    ndt_out = [float(ndt.linearize(np.eye(4))[0]), oc._ndt_voxels(ndt, 0)]
    v = c.view("vgicp")
    oc.route(c)
    v.setInputTargetDevice(dc_map.ptr.value, len(dc_map), 16); v.setInputSourceDevice(dc_scan.ptr.value, len(dc_scan), 16)
    v.align(np.eye(4, dtype=np.float32), want_output=False, want_fitness=True)
    vg_out = oc._solve_out(v, fitness=v.getFitnessScore())
    icp = c.view("icp"); icp.setInputSource(dc_scan); icp.setInputTarget(dc_map)
    icp_out = [icp.align().copy(), float(icp.getFitnessScore()), int(icp.nr_iterations)]
    h_map, h_scan = dc_map.numpy(), dc_scan.numpy()
    assert len(h_map) > 2000 and len(h_scan) > 500

    def kf_alone(a):
        s = oc._kf_fill(a, drive)
        return [s.assemble(drive["ids"][:8], (2,), leaf=0.3).copy(), s.assemble(drive["ids"][8:10], (1,)).copy()]
    _same([h_map, h_scan], _alone(kf_alone), "rgc_kf_assemble(on_device)", c)

    def search_alone(a):
        t = a.view("tree"); t.setInputCloud(h_map)
        return list(t.nearestKSearch(qry, 8))
    _same(knn, _alone(search_alone), "rgc_search_set_cloud(on_device) on the assembled cloud", c)

    def ndt_alone(a):
        o = a.view("ndt"); o.setResolution(1.0); o.setDistanceMode(p.ndt.NDT_D2D); o.setNeighborSearchMethod(p.ndt.NDT_DIRECT7)
        o.setInputTarget(h_map); o.setInputSource(h_scan)
        return [float(o.linearize(np.eye(4))[0]), oc._ndt_voxels(o, 0)]
    _same(ndt_out, _alone(ndt_alone), "rgc_ndt_set_target_device on the assembled cloud", c)

    def vgicp_alone(a):
        oc.route(a)
        a.v.setInputTarget(h_map); a.v.setInputSource(h_scan)
        a.v.align(np.eye(4, dtype=np.float32), want_output=False, want_fitness=True)
        return oc._solve_out(a.v, fitness=a.v.getFitnessScore())
    _same(vg_out, _alone(vgicp_alone), "rgc_set_target_device + align on the assembled cloud", c)

    def icp_alone(a):
        o = a.view("icp"); o.setInputSource(h_scan); o.setInputTarget(h_map)
        return [o.align().copy(), float(o.getFitnessScore()), int(o.nr_iterations)]
    _same(icp_out, _alone(icp_alone), "rgc_icp_align_device on two assembled clouds", c)
    _chain_3(c, sweep)



# ---- a solve in flight ----------------------------------------------------------------------------------------------------------------------------------------------
class _SentinelNumpy:
    """numpy for the package's wrappers during a call that must be refused: every array a wrapper allocates for the library to write (np.empty, np.zeros)
    is filled with a sentinel and remembered; the rest is numpy's.  It sees what the package's wrappers allocate; _refused_calls below fills the outputs of
    raw calls itself, entry point by entry point"""

    def __init__(self):
        self.made = []

    def __getattr__(self, name):
        return getattr(np, name)

    def _fill(self, a):
        a.reshape(-1).view(np.uint8)[:] = oc.SENTINEL
        self.made.append(a)
        return a

    def empty(self, *a, **k):
        return self._fill(np.empty(*a, **k))

    def zeros(self, *a, **k):
        return self._fill(np.zeros(*a, **k))

    def untouched(self):
        return all(bool((a.reshape(-1).view(np.uint8) == oc.SENTINEL).all()) for a in self.made)


def _infos(c):
    """every info record that can be read with a solve in flight"""
    lib, L = oc.P()._lib, c.L
    out = {}
    for key, fn, rec in (("search", L.rgc_search_get_info, lib.SearchInfo), ("outlier", L.rgc_outlier_get_info, lib.OutlierInfo), ("cluster", L.rgc_cluster_get_info, lib.ClusterInfo),
                         ("plane", L.rgc_plane_get_info, lib.PlaneInfo), ("normal", L.rgc_normal_get_info, lib.NormalInfo), ("fpfh", L.rgc_fpfh_get_info, lib.FpfhInfo),
                         ("map", L.rgc_map_get_info, lib.MapInfo), ("kf", L.rgc_kf_get_info, lib.KfInfo), ("vg_route", L.rgc_voxelgrid_route, lib.VgRoute)):
        r = rec()
        c.chk(fn(c.h, C.byref(r)))
        out[key] = bytes(r)
    return out


def _refused_calls(c, inp, dev):
    """every entry point the header refuses with a solve in flight, called raw with valid arguments and sentinel-filled outputs: (name, call) pairs, call()
    -> (status, the output arrays).  `dev`: device buffers uploaded before the solve began"""
    lib, L, h = oc.P()._lib, c.L, c.h
    fp, dp, ip = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int)
    made = []

    def S(shape, dtype=np.float64):
        a = np.empty(shape, dtype)
        a.reshape(-1).view(np.uint8)[:] = oc.SENTINEL
        made.append(a)
        return a
    tgt, src, n = inp["tgt"], inp["src"], len(inp["src"])
    T64, T32 = np.ascontiguousarray(inp["T_a"], np.float64), np.eye(4, dtype=np.float32)
    q, t3 = np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3)
    plane_cov = np.tile(np.diag([1.0, 1.0, 0.001]).reshape(1, 9), (n, 1))
    prm = lib.Params()
    c.chk(L.rgc_get_params(h, C.byref(prm)))
    prm.voxel_res *= 0.5
    mp = lib.GicpMpParams()
    c.chk(L.rgc_gicpmp_get_params(h, C.byref(mp)))
    pl, nr, fh = lib.PlaneParams(), lib.NormalParams(), lib.FpfhParams()
    L.rgc_default_plane_params(C.byref(pl)); pl.distance_threshold = 0.1
    nr.k, nr.flip = 8, 1
    fh.radius = 0.5
    i1 = lambda: S(1, np.int32)            # noqa: E731
    d = lambda a: a.ctypes.data_as(dp)     # noqa: E731
    f = lambda a: a.ctypes.data_as(fp)     # noqa: E731
    i = lambda a: a.ctypes.data_as(ip)     # noqa: E731
    solve = lambda fn: lambda: fn(h, f(T32), f(S(16, np.float32)), d(S(36)), d(S(1)), i(i1()), i(i1()), i(i1()))      # noqa: E731
    lin = lambda fn: lambda: fn(h, d(T64), d(S(36)), d(S(6)), d(S(1)))                                                 # noqa: E731
    calls = [
        ("rgc_set_target", lambda: L.rgc_set_target(h, tgt.ctypes.data, len(tgt), 12)), ("rgc_set_source", lambda: L.rgc_set_source(h, src.ctypes.data, n, 12)),
        ("rgc_set_target_device", lambda: L.rgc_set_target_device(h, dev["tgt"].ptr, len(tgt), 12)),
        ("rgc_set_source_device", lambda: L.rgc_set_source_device(h, dev["src"].ptr, n, 12)),
        ("rgc_set_target_reframed", lambda: L.rgc_set_target_reframed(h, dev["map"].ptr, len(tgt), 16, d(q), d(t3), dev["body"].ptr)),
        ("rgc_set_params", lambda: L.rgc_set_params(h, C.byref(prm))), ("rgc_set_neighbor_search", lambda: L.rgc_set_neighbor_search(h, oc.DIRECT7, -1.0)),
        ("rgc_set_target_lazy", lambda: L.rgc_set_target_lazy(h, 2)), ("rgc_set_regularization_method", lambda: L.rgc_set_regularization_method(h, 4)),
        ("rgc_set_voxel_accumulation_mode", lambda: L.rgc_set_voxel_accumulation_mode(h, 2)), ("rgc_set_covariance_estimation", lambda: L.rgc_set_covariance_estimation(h, 1)),
        ("rgc_linearize", lin(L.rgc_linearize)), ("rgc_align", solve(L.rgc_align)), ("rgc_align_begin", lambda: L.rgc_align_begin(h, f(T32), 0)),
        ("rgc_get_source_covariances", lambda: L.rgc_get_source_covariances(h, d(S((n, 9))), None)),
        ("rgc_get_target_covariances", lambda: L.rgc_get_target_covariances(h, d(S((len(tgt), 9))), None)),
        ("rgc_get_voxels", lambda: L.rgc_get_voxels(h, 0, None, None, None, None, i(i1()))),
        ("rgc_set_source_covariances", lambda: L.rgc_set_source_covariances(h, d(plane_cov), n)),
        ("rgc_swap_source_and_target", lambda: L.rgc_swap_source_and_target(h)), ("rgc_clear_source", lambda: L.rgc_clear_source(h)),
        ("rgc_clear_target", lambda: L.rgc_clear_target(h)),
        ("rgc_gicp_linearize", lin(L.rgc_gicp_linearize)), ("rgc_gicp_compute_error", lambda: L.rgc_gicp_compute_error(h, d(T64), d(S(1)))),
        ("rgc_gicp_num_correspondences", lambda: L.rgc_gicp_num_correspondences(h, i(i1()))),
        ("rgc_gicp_get_correspondences", lambda: L.rgc_gicp_get_correspondences(h, i(S(n, np.int32)), f(S(n, np.float32)))), ("rgc_gicp_align", solve(L.rgc_gicp_align)),
        ("rgc_gicpst_linearize", lin(L.rgc_gicpst_linearize)), ("rgc_gicpst_compute_error", lambda: L.rgc_gicpst_compute_error(h, d(T64), d(S(1)))),
        ("rgc_gicpst_reset", lambda: L.rgc_gicpst_reset(h)), ("rgc_gicpst_align", solve(L.rgc_gicpst_align)),
        ("rgc_gicpmp_set_params", lambda: L.rgc_gicpmp_set_params(h, C.byref(mp))), ("rgc_gicpmp_linearize", lin(L.rgc_gicpmp_linearize)),
        ("rgc_gicpmp_align", solve(L.rgc_gicpmp_align)),
        ("rgc_search_set_cloud", lambda: L.rgc_search_set_cloud(h, tgt.ctypes.data, len(tgt), 12, 0, 0.0)), ("rgc_search_clear", lambda: L.rgc_search_clear(h)),
        ("rgc_search_knn", lambda: L.rgc_search_knn(h, src.ctypes.data, n, 12, 0, 5, S((n, 5), np.int32).ctypes.data, S((n, 5), np.float32).ctypes.data)),
        ("rgc_search_radius", lambda: L.rgc_search_radius(h, src.ctypes.data, n, 12, 0, 0.5, 0, 1, S(n + 1, np.int32).ctypes.data, S(64, np.int32).ctypes.data,
                                                          S(64, np.float32).ctypes.data, 64, C.byref(C.c_longlong(0)))),
        ("rgc_outlier_statistical", lambda: L.rgc_outlier_statistical(h, src.ctypes.data, n, 12, 0, 8, 1.0, 0, S((n, 4), np.float32).ctypes.data, S(n, np.int32).ctypes.data,
                                                                      S(n, np.float32).ctypes.data, i(i1()))),
        ("rgc_outlier_radius", lambda: L.rgc_outlier_radius(h, src.ctypes.data, n, 12, 0, 0.5, 3, 0, S((n, 4), np.float32).ctypes.data, S(n, np.int32).ctypes.data,
                                                            S(n, np.int32).ctypes.data, i(i1()))),
        ("rgc_cluster_extract", lambda: L.rgc_cluster_extract(h, src.ctypes.data, n, 12, 0, 0.5, 1, 2 ** 31 - 1, S(n, np.int32).ctypes.data, S(n + 1, np.int32).ctypes.data,
                                                              S(n, np.int32).ctypes.data, i(i1()))),
        ("rgc_plane_segment", lambda: L.rgc_plane_segment(h, src.ctypes.data, n, 12, 0, C.byref(pl), None, 0, 0, S(4).ctypes.data, S((n, 4), np.float32).ctypes.data,
                                                          S(n, np.int32).ctypes.data, None, i(i1()))),
        ("rgc_normal_estimate", lambda: L.rgc_normal_estimate(h, src.ctypes.data, n, 12, None, 0, 0, 0, C.byref(nr), S((n, 4), np.float32).ctypes.data, S((n, 6)).ctypes.data,
                                                              S((n, 3)).ctypes.data, S(n, np.int32).ctypes.data, i(i1()))),
        ("rgc_fpfh_estimate", lambda: L.rgc_fpfh_estimate(h, src.ctypes.data, n, 12, None, 0, 0, tgt.ctypes.data, 12, 0, C.byref(fh), S((n, 33), np.float32).ctypes.data,
                                                          S((n, 33), np.uint32).ctypes.data, S(n, np.int32).ctypes.data, S(n, np.int32).ctypes.data, i(i1()))),
        ("rgc_map_commit", lambda: L.rgc_map_commit(h, C.c_float(0.3), i(i1()))),
    ]
    return calls, made


@pytest.mark.parametrize("reg", [oc.REG_PLANE, oc.REG_MIN_EIG], ids=["tuned_route", "general_route"])
def test_a_solve_in_flight_for_every_operation(lone, ctx, monkeypatch, reg):
    """between rgc_align_begin and rgc_align_end every operation once: a refused one returns RGC_ERR_INVALID, writes no output array and no info record; one
    that runs equals its lone result; rgc_align_end then returns the bytes of the undisturbed solve"""
    import rgc_slam_amd
    lib = oc.P()._lib
    modules = [m for m in vars(rgc_slam_amd).values() if getattr(m, "np", None) is np]
    assert len(modules) >= 10
    for name in NAMES:                                       # (state of every subsystem on the context before the solve, so that a refusal has something to spoil)
        oc.check(ctx, name, "small", _first(name))
    inp = oc.reg_inputs("small")
    a4 = np.zeros((len(inp["tgt"]), 4), np.float32)
    a4[:, :3] = inp["tgt"]
    dev = dict(tgt=oc.Dev(ctx, inp["tgt"]), src=oc.Dev(ctx, inp["src"]), map=oc.Dev(ctx, a4), body=oc.Dev(ctx, np.zeros_like(a4)))     # (before the solve begins)
    ctx.hold("in_flight", list(dev.values()))
    oc.solve_begin(ctx, inp, reg=reg)
    for name in NAMES:
        o = oc.OPS[name]
        if o.in_flight == "runs":
            oc.check(ctx, name, "small", _first(name), what="with a solve in flight")
            continue
        # the operation as a caller writes it: nothing is selected with a solve in flight (route()), so its OWN first entry point answers
        before, proxy = _infos(ctx), _SentinelNumpy()
        with monkeypatch.context() as mp:
            for m in modules:
                mp.setattr(m, "np", proxy)
            with pytest.raises(lib.RgcError) as e:
                o.run(ctx, "small", "host" if "host" in o.forms else o.forms[0])
        assert e.value.status == lib.ERR_INVALID and "in flight" in str(e.value), "%s: %s\nhistory: %s" % (name, e.value, " -> ".join(ctx.history))
        assert proxy.untouched(), "%s was refused and wrote into an output array\nhistory: %s" % (name, " -> ".join(ctx.history))
        after = _infos(ctx)
        changed = [k for k in before if before[k] != after[k] and not (k == "map" and not o.refused_whole)]
        assert not changed, "%s was refused and changed the info records %s\nhistory: %s" % (name, changed, " -> ".join(ctx.history))
        if not o.refused_whole:                  # rgc_map_reset / rgc_map_insert ran, rgc_map_commit was refused 'before a byte is written'
            m = ctx.view("map")
            info = m.info()
            assert before["map"] != after["map"] and info["n_keyframes"] == 3 and info["n_target"] == -1, info
            assert oc.same(m.points(), lone("map_insert_evict_rebase", "small", "host")["points"]), "the map the refused commit left"
    # every refused entry point on its own, raw: the status, the message, the outputs and the info records
    calls, made = _refused_calls(ctx, inp, dev)
    covered = set().union(*[oc.OPS[n].covers for n in NAMES if oc.OPS[n].in_flight == "refused"])
    assert {n for n, _ in calls} <= covered
    before = _infos(ctx)
    for name, call in calls:
        ctx.history.append(name + " (raw)")
        rc = call()
        msg = ctx.L.rgc_last_error(ctx.h).decode()
        assert rc == lib.ERR_INVALID and "in flight" in msg, "%s with a solve in flight: status %d, '%s'\nhistory: %s" % (name, rc, msg, " -> ".join(ctx.history[-6:]))
        assert all(bool((a.reshape(-1).view(np.uint8) == oc.SENTINEL).all()) for a in made), "%s was refused and wrote into an output" % name
        assert _infos(ctx) == before, "%s was refused and changed an info record" % name
    got = oc.solve_end(ctx)
    bad = oc.diff(got, oc.lone_solve("small", reg))
    assert not bad, "the solve in flight across every operation differs from the undisturbed solve at %s\nhistory: %s" % (bad, " -> ".join(ctx.history))


# ---- profiling ---------------------------------------------------------------------------------------------------------------------------------------------------------
def test_profiling_changes_no_byte(lone, ctx):
    ctx.chk(ctx.L.rgc_profile_enable(ctx.h, 1))
    for name in NAMES:
        oc.check(ctx, name, "small", _first(name), what="with profiling on")
    ctx.chk(ctx.L.rgc_profile_enable(ctx.h, 0))
    oc.check(ctx, "vgicp_direct1", "small", "host", what="profiling switched off again")
    oc.check(ctx, "vgicp_align_in_halves", "small", "device", what="profiling switched off again")


# ---- seeded schedules -----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [11, 12, 13])
def test_seeded_schedules(lone, ctx, seed):
    """60 operations drawn at random (operation, size, form); a leaf filter is sometimes left open across the next one to three operations, a solve sometimes
    left in flight across the next operation; every result against lone, every kept record at the end.  python tests/one_context_ops.py runs longer ones"""
    sched = oc.schedule(seed, 60)
    try:
        assert oc.run_schedule(ctx, sched) >= 60
    except AssertionError as e:
        raise AssertionError("seed %d, schedule %s\n%s" % (seed, [s[:3] for s in sched], e)) from None


# ---- threads ---------------------------------------------------------------------------------------------------------------------------------------------------------------
FEATURES = ["search_knn", "search_radius", "outlier_statistical", "outlier_radius", "cluster_extract", "plane_segment", "normals_k", "normals_radius", "fpfh", "ndt_p2d",
            "ndt_d2d", "kf_push_assemble", "kf_select"]


def test_threads_on_contexts_of_their_own(lone):
    """four host threads in one process, a context each, a different rotation of the feature operations each: all results equal lone"""
    for name in FEATURES:
        lone(name, "small", "host")
    errors = []

    def work(t):
        c = oc.Ctx()
        try:
            for k in range(len(FEATURES)):
                oc.check(c, FEATURES[(3 * t + k) % len(FEATURES)], "small", "host", what="thread %d" % t)
        except BaseException as e:          # noqa: B902  (reported by the main thread)
            errors.append("thread %d: %s" % (t, e))
        finally:
            c.close()
    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, "\n".join(errors)
