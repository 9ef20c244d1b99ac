"""The operation table of the one-context tests: every subsystem of include/rgc_hip.h as an operation that can run on a context it shares with all
the others (rgc::OdometryNode, odometry.Preprocessor and the owner= parameter of the Python classes put several subsystems on one rgc_ctx).

One entry per operation (OPS, a dict by name of Op records):
  covers     the rgc_* entry points the operation calls (tests/test_one_context_table.py holds their union against the header: a new entry point
             fails that test until it joins an operation here, or EXCLUDED with a reason)
  sizes      {"small": ..., "large": ...}: which designed case each size is.  `small` is the smallest case of the feature's module that still takes more
             than one workgroup (and the cube-growth path where the kernel has one); `large` has at least four times its points, so that every
             DevBuf the operation uses is reallocated by ensure() when `large` follows `small` on one context (an entry that cannot meet this says
             EXCEPTION in its `large` text; `points(inputs)` counts them and tests/test_one_context_table.py holds the ratio)
  forms      "host" and / or "device": for "device" the inputs are uploaded with rgc_upload into the SAME context, handed over as device memory
             without a synchronisation, and what the call leaves in device buffers is downloaded afterwards
  make       make(size) -> the inputs (cached, read-only)
  run        run(ctx, inputs, form) -> a dict of every output array, scalar and info record of the operation
  kept       kept(ctx) -> what the operation left on the context, read back (the search index's answers to fixed queries, voxel maps, covariances, a
             frozen cost, the store's info and an assemble, the map's points, each feature's *_get_info ...)
  reads      the state groups `kept` reads;  writes: the state groups the operation replaces.  kept(A) must be unchanged after B unless
             B.writes meets A.reads -- the exceptions the header states, collected in GROUPS below with the sentence they come from
  in_flight  "refused" or "runs": what include/rgc_hip.h says the operation does between rgc_align_begin and rgc_align_end

An operation is self-contained: it selects every context-wide setting its result depends on (the neighbour method, the regularisation, the covariance
estimation, NDT's and MultiPoints' parameters), sets its own clouds and runs.  The context's rgc_params block is the odometer's and is never left
changed (rgc_set_params is refused with a solve in flight, and NDT, ICP and the GICP variants read their LM settings from it).

All comparisons are of bytes (same() below).  Where the header does not promise an order the table says so and the wrapper sorts: rgc_get_voxels and
rgc_ndt_get_voxels are "unordered" dumps (sorted here by voxel coordinates), nothing else.

The library is imported lazily (P()), so that the CPU test can import this module on a machine without librgc_hip.so.

    python tests/one_context_ops.py [trials] [seed] [operations per trial]      # longer seeded campaigns by hand, as the scripts of tests/fuzz do"""
import ctypes as C
import functools
import json
import os
import struct
import sys
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

SIZES = ("small", "large")
SENTINEL = 0x5A


@functools.lru_cache(maxsize=None)
def P():
    """the package, imported on first use"""
    import rgc_slam_amd  # noqa: F401
    from rgc_slam_amd import (_lib, features, filters, frontend, gicp, keyframes, local_map, loop_closure, mapping, ndt, odometry, pose_graph, registration,
                              search, segmentation, synth, wire)
    return types.SimpleNamespace(_lib=_lib, features=features, filters=filters, frontend=frontend, gicp=gicp, keyframes=keyframes, local_map=local_map,
                                 loop_closure=loop_closure, mapping=mapping, ndt=ndt, odometry=odometry, pose_graph=pose_graph, registration=registration,
                                 search=search, segmentation=segmentation, synth=synth, wire=wire)


# ---- state groups: what a kept record reads and what an operation replaces, with the header's sentence ------------------------------------------------
GROUPS = {
    "reg": "the context's own source and target, their covariances, the voxel map and every frozen linearisation on them: 'Setting a cloud drops its "
           "covariances (and, for the target, the voxel map)'; drop_frozen (rgc_ctx.h): VGICP's correspondences and the state of FastGICP, SingleThread and "
           "MultiPoints 'fall together wherever a cloud is set, cleared, swapped, shared, given covariances or prepared again'; rgc_map_commit 'makes the map "
           "the registration target'; a changed regularisation / covariance method 'DROPS the clouds'",
    "search": "the search index: rgc_search_set_cloud replaces it, rgc_search_clear drops it; every other subsystem leaves it untouched",
    "search_info": "rgc_search_info: 'the search index and what its last query call cost'",
    "ndt": "NDT's clouds and voxel maps: 'a block of its own on the context'; rgc_ndt_set_* / clear / swap replace them",
    "kf": "the keyframe store: rgc_kf_reset / push / set_poses and rgc_pgo_optimize with apply change it",
    "map": "the resident map: rgc_map_reset / insert / evict / rebase / commit change it",
    "mapreg": "the mapping registration's two maps: rgc_mapreg_set_maps* replaces them",
    "vg_route": "rgc_voxelgrid_route: 'filled by every rgc_voxelgrid and rgc_voxelgrid_end', by rgc_uniform_sampling ('rgc_voxelgrid_route reports it'), and "
                "through them by rgc_kf_assemble with a leaf, the two selections and rgc_map_commit",
    "outlier_info": "rgc_outlier_info: 'the last outlier filter call'",
    "cluster_info": "rgc_cluster_info: 'the last rgc_cluster_extract'",
    "plane_info": "rgc_plane_info: 'the last rgc_plane_segment'",
    "normal_info": "rgc_normal_info: 'the last rgc_normal_estimate'",
    "fpfh_info": "rgc_fpfh_info: 'the last rgc_fpfh_estimate'",
}

# entry points that take a context first and are in no operation, with the reason
EXCLUDED = {
    "rgc_destroy": "life-cycle: every context of the tests ends with it",
    "rgc_last_error": "pure getter: the message of the last failure, read by every wrapper",
    "rgc_get_neighbor_search": "pure getter of a setting",
    "rgc_get_covariance_estimation": "pure getter of a setting",
    "rgc_get_rbf_kernel": "pure getter of a setting",
    "rgc_get_knn_reuse": "pure getter of a setting",
    "rgc_ndt_get_params": "pure getter of a setting",
    "rgc_gicp_get_max_correspondence_distance": "pure getter of a setting",
    "rgc_gicpmp_get_params": "pure getter of a setting",
    "rgc_device_alloc": "allocation: used by every device-form operation",
    "rgc_device_free": "allocation: used by every device-form operation",
    "rgc_upload": "transfer: used by every device-form operation",
    "rgc_download": "transfer: used by every device-form operation",
    "rgc_synchronize": "waits for the context's stream; the tests add no synchronisation of their own",
    "rgc_stream": "pure getter: the context's stream handle",
    "rgc_get_stats": "read-out of counters that accumulate over a context's life (they differ between a shared context and a lone one by design)",
    "rgc_profile_enable": "profiling: switched by test_profiling_changes_no_byte around every operation",
    "rgc_profile_select": "profiling read-out",
    "rgc_profile_reset": "profiling read-out",
    "rgc_profile_get": "profiling read-out",
    "rgc_share_target": "works between TWO contexts (tests/test_gpu_sequence.py, test_gpu_rolling_map.py)",
    "rgc_hold_source_until_target_of": "works between TWO contexts: a scheduling hint, results unaffected",
    "rgc_outlier_set_cell": "tuning knob for tests: 'no output depends on it'",
    "rgc_cluster_set_cell": "tuning knob for tests: 'no output depends on it'",
    "rgc_normal_set_cell": "tuning knob for tests (0 = automatic, what every operation here runs with)",
    "rgc_fpfh_set_cell": "tuning knob for tests (0 = automatic, what every operation here runs with)",
    "rgc_plane_set_batch": "tuning knob for tests: 'no output depends on it'",
}


# ---- bytes ---------------------------------------------------------------------------------------------------------------------------------------------
def _b(v):
    if isinstance(v, np.ndarray):
        return (str(v.dtype), v.shape, np.ascontiguousarray(v).tobytes())
    if isinstance(v, (float, np.floating)):
        return ("f8", struct.pack("<d", float(v)))
    if isinstance(v, (bool, np.bool_)):
        return ("b", bool(v))
    if isinstance(v, (int, np.integer)):
        return ("i", int(v))
    return ("o", v)


def diff(a, b, path=""):
    """the paths at which two results differ in a byte (arrays as bytes with dtype and shape, floats as their 8 bytes, NaN included)"""
    if isinstance(a, dict) and isinstance(b, dict):
        out = [path + "/" + str(k) + " (missing)" for k in set(a) ^ set(b)]
        for k in a:
            if k in b:
                out += diff(a[k], b[k], path + "/" + str(k))
        return out
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        if len(a) != len(b):
            return [path + " (length %d / %d)" % (len(a), len(b))]
        return sum((diff(x, y, path + "[%d]" % i) for i, (x, y) in enumerate(zip(a, b))), [])
    if _b(a) == _b(b):
        return []
    note = ""
    if isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.shape == b.shape and a.dtype == b.dtype and a.size:      # (for the message only)
        ne = a.view(np.uint8).reshape(a.size, -1) != b.view(np.uint8).reshape(b.size, -1) if a.flags.c_contiguous and b.flags.c_contiguous else None
        if ne is not None and a.dtype.kind == "f":
            with np.errstate(all="ignore"):
                note = " [%d of %d elements, max |d| = %.3g]" % (int(ne.any(axis=1).sum()), a.size, float(np.nanmax(np.abs(a.astype(np.float64) - b.astype(np.float64)))))
        elif ne is not None:
            note = " [%d of %d elements]" % (int(ne.any(axis=1).sum()), a.size)
    elif isinstance(a, (float, int)) and isinstance(b, (float, int)):
        note = " [%r / %r]" % (a, b)
    return [(path or "/") + note]


def same(a, b):
    return not diff(a, b)


def _ro(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


# ---- a context every subsystem lives on ----------------------------------------------------------------------------------------------------------------
def share(obj, owner):
    """obj gives up its own context and works on owner's (tests/fuzz/fuzz_one_context.py's handle swap, for the classes without owner=)"""
    obj._L.rgc_destroy(obj._h)
    obj._h = owner._h
    obj.close = lambda: None
    return obj


class Dev:
    """a host array uploaded into the context with rgc_upload (asynchronous, stream-ordered: nothing waits for it); quacks like keyframes.DeviceCloud"""

    def __init__(self, ctx, a, dtype=np.float32):
        self.a = np.ascontiguousarray(a, dtype)            # alive until free(): the copy is asynchronous
        self._L, self._h, self._ctx = ctx.L, ctx.h, ctx
        self.ptr = C.c_void_p()
        ctx.chk(self._L.rgc_device_alloc(self._h, max(self.a.nbytes, 16), C.byref(self.ptr)))
        if self.a.nbytes:
            ctx.chk(self._L.rgc_upload(self._h, self.ptr, self.a.ctypes.data, self.a.nbytes))
        self.n = self.a.shape[0]

    def __len__(self):
        return self.n

    @property
    def stride_bytes(self):
        return self.a.strides[0]

    @property
    def addr(self):
        return self.ptr.value

    def synchronize(self):
        self._ctx.chk(self._L.rgc_synchronize(self._h))

    def numpy(self, shape=None, dtype=None):
        out = np.empty(self.a.shape if shape is None else shape, self.a.dtype if dtype is None else dtype)
        if out.nbytes:
            self._ctx.chk(self._L.rgc_download(self._h, out.ctypes.data, self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            self._L.rgc_device_free(self._h, self.ptr)
            self.ptr = None


class Ctx:
    """one rgc_ctx and a view of every Python class on it: through owner= where the class has it, through share() otherwise"""

    def __init__(self):
        p = P()
        self.v = p.registration.odometer_vgicp(0)
        self.L, self.h = self.v._L, self.v._h
        self._views = {"vgicp": self.v}
        self._held = {}
        self.history = []
        self.in_flight = False                              # between solve_begin and solve_end
        self.vg_open, self.vg_size = None, None             # rgc_voxelgrid_begin's buffers while the filter is left open

    def chk(self, rc):
        if rc != 0:
            raise P()._lib.RgcError(rc, self.L.rgc_last_error(self.h).decode() or self.L.rgc_status_string(rc).decode())

    def view(self, name):
        if name in self._views:
            return self._views[name]
        p, v = P(), self.v
        make = {
            "gicp": lambda: share(p.gicp.FastGICP(0), v), "gicpst": lambda: share(p.gicp.FastGICPSingleThread(0), v),
            "gicpmp": lambda: share(p.gicp.FastGICPMultiPoints(0), v), "pre": lambda: share(p.odometry.Preprocessor(0), v),
            "fe": lambda: share(p.frontend.ScanRegistration(16), v), "wire": lambda: share(p.wire.Wire(0), v),
            "icp": lambda: share(p.loop_closure.IterativeClosestPoint(0), v), "mapreg": lambda: share(p.mapping.MapFeatureRegistration(0), v),
            "ndt": lambda: p.ndt.NDTRegistration(owner=v), "tree": lambda: p.search.KdTree(owner=v),
            "sor": lambda: p.filters.StatisticalOutlierRemoval(owner=v), "ror": lambda: p.filters.RadiusOutlierRemoval(owner=v),
            "cluster": lambda: p.segmentation.EuclideanClusterExtraction(owner=v), "plane": lambda: p.segmentation.SACSegmentation(owner=v),
            "normal": lambda: p.features.NormalEstimation(owner=v), "fpfh": lambda: p.features.FPFHEstimation(owner=v),
            "store": lambda: p.keyframes.KeyframeStore(owner=v), "map": lambda: p.local_map.RollingLocalMap(v),
        }[name]
        self._views[name] = make()
        return self._views[name]

    def hold(self, group, bufs):
        """device inputs a subsystem may read again later (a speculative grid prepares a cloud again from where it was set) live until the next
        operation replaces them"""
        for b in self._held.pop(group, []):
            b.free()
        self._held[group] = list(bufs)

    def close(self):
        if self.v._h is None:
            return
        self.L.rgc_synchronize(self.h)
        for g in list(self._held):
            self.hold(g, [])
        for name, o in self._views.items():
            if o is not self.v and hasattr(o, "_h"):
                o._h = None
        self.v.close()


def up(ctx, form, a, bufs, dtype=np.float32):
    """the array itself for the host form, a Dev (remembered in bufs) for the device form"""
    if form == "host":
        return np.ascontiguousarray(a, dtype)
    d = Dev(ctx, a, dtype)
    bufs.append(d)
    return d


def free(bufs):
    for b in bufs:
        b.free()


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------------------
def _quat(R):
    qw = np.sqrt(1 + np.trace(R)) / 2
    return np.array([(R[2, 1] - R[1, 2]) / (4 * qw), (R[0, 2] - R[2, 0]) / (4 * qw), (R[1, 0] - R[0, 1]) / (4 * qw), qw])


@functools.lru_cache(maxsize=None)
def _world():
    return P().synth.make_world(half_extent=40.0, seed=4242)


REG_N = {"small": (5000, 1250), "large": (20000, 5000)}      # (fuzz_null_args.py's and smoke()'s clouds)


@functools.lru_cache(maxsize=None)
def reg_inputs(size):
    """a map and a scan of it a small motion away (synth, at the sizes of smoke() and the fuzz scripts), the poses the seams are evaluated at"""
    s = P().synth
    nt, ns = REG_N[size]
    world, tgt = s.make_world_and_map(nt, seed=4300)
    T_true = s.se3(s.rot_zyx(0.02, 0.002, -0.001), [0.12, 0.02, 0.001])
    src = s.make_scan_n(world, T_true, ns, seed=4301)["xyz"]
    T_a = s.se3(s.rot_zyx(0.015, 0.001, 0.0), [0.1, 0.01, 0.0]).astype(np.float64)
    T_b = s.se3(s.rot_zyx(0.025, 0.0, -0.002), [0.14, 0.03, 0.002]).astype(np.float64)
    return _ro(dict(tgt=np.ascontiguousarray(tgt, np.float32), src=np.ascontiguousarray(src, np.float32), T_a=T_a, T_b=T_b, guess=np.eye(4, dtype=np.float32)))


SCAN_AZ = {"small": 300, "large": 1500}


@functools.lru_cache(maxsize=None)
def scan_inputs(size, n_az=None, seed=4400):
    """a synthetic sweep as the front-end encodes it (x, y, z, ring + 0.1 relTime) and raw (x, y, z, intensity), a motion and a re-framing pose"""
    s = P().synth
    rng = np.random.default_rng(seed)
    T = s.se3(s.rot_zyx(0.3, 0.004, -0.003), [1.5, -0.8, 0.01])
    sc = s.make_scan(_world(), T, n_az=n_az or SCAN_AZ[size], seed=seed + 1)
    xyzi = np.concatenate([sc["xyz"], (sc["ring"] + 0.1 * sc["rel_time"])[:, None]], axis=1).astype(np.float32)
    raw = np.concatenate([sc["xyz"], sc["intensity"][:, None]], axis=1).astype(np.float32)
    q_motion, t_motion = _quat(s.rot_zyx(0.012, -0.004, 0.006)), rng.normal(0, 0.2, 3)
    q = rng.normal(0, 1, 4)
    return _ro(dict(xyzi=xyzi, raw=raw, q_motion=q_motion, t_motion=t_motion, q=q / np.linalg.norm(q), t=rng.uniform(-30, 30, 3)))


@functools.lru_cache(maxsize=None)
def drive_inputs(size):
    """keyframes of a synthetic drive: body-frame sweeps as the three cloud kinds (every 7th / 3rd point / all), key poses that re-enter their first side
    (us_cases.square_drive), the loop edges of pgo_cases between them"""
    import us_cases
    p = P()
    n_kf, n_az = 12, {"small": 60, "large": 260}[size]
    poses, ids = us_cases.square_drive(n=248, side_steps=60, step=0.5)
    sel = np.r_[0:6, 240:246]                                # the first poses and the ones that lie where they do, one lap later
    clouds = []
    for j, k in enumerate(sel):
        x, y, yaw = float(poses[k, 0]) * 0.1, float(poses[k, 1]) * 0.1, float(poses[k, 5])
        T = p.synth.se3(p.synth.rot_zyx(yaw, 0.0, 0.0), [x, y, 0.0])
        sc = p.synth.make_scan(_world(), T, n_az=n_az, seed=4500 + j)
        a = np.concatenate([sc["xyz"], sc["intensity"][:, None]], axis=1).astype(np.float32)
        clouds.append((np.ascontiguousarray(a[::7]), np.ascontiguousarray(a[::3]), a))
    kp = poses[sel].copy()
    kp[:, :2] *= np.float32(0.1)
    moved = kp[3:9].copy()
    moved[:, :3] += np.float32(0.03125)
    return _ro(dict(ids=np.arange(n_kf, dtype=np.int32) * 3 + 5, poses=kp, moved_ids=(np.arange(3, 9, dtype=np.int32) * 3 + 5), moved=moved)) | dict(clouds=clouds)


# ---- the registration's route, selected by every operation on the context's own clouds ----------------------------------------------------------------------
ROUTE_COVERS = {"rgc_get_params", "rgc_set_params", "rgc_set_source", "rgc_clear_source", "rgc_set_neighbor_search", "rgc_set_regularization_method", "rgc_set_voxel_accumulation_mode", "rgc_set_covariance_estimation", "rgc_set_rbf_kernel",
                "rgc_set_target_lazy"}
CLOUD_COVERS = {"rgc_set_target", "rgc_set_source", "rgc_set_target_device", "rgc_set_source_device"}
DIRECT27, DIRECT7, DIRECT1, DIRECT_RADIUS = 0, 1, 2, 3
REG_PLANE, REG_MIN_EIG = 3, 1


_DUMMY_SCAN = (np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij"), axis=-1).reshape(-1, 3) * 0.25).astype(np.float32)


def route(ctx, method=DIRECT1, radius=-1.0, reg=REG_PLANE, cov=0, rbf=(0.5, 3.0)):
    """every context-wide setting a registration on the context's own clouds depends on.  The first is no setting: the SCAN's kNN grid.  Its cell size
    follows how crowded the previous scan's cells were on this context, and its box is kept from the previous scans while the next one fits it; the box
    decides which far-field points go to the cooperative kernel, which sums their moments in another order than the four-lane search, so the last bits of
    the source covariances (and of cost, H, b) depend on the scans a context has seen (include/rgc_hip.h at rgc_set_source).  Put back to
    where a context of its own starts: rgc_set_params with another voxel_res resets the cell size; a 64-point scan set at that other resolution and
    cleared leaves a kept box of another resolution, which the next scan does not use -- its own box is measured, as on a new context.
    With a solve in flight nothing is selected: every call below is refused then, and the operation's own first entry point is what must answer."""
    if ctx.in_flight:
        return
    L, h = ctx.L, ctx.h
    p = P()._lib.Params()
    ctx.chk(L.rgc_get_params(h, C.byref(p)))
    res = p.voxel_res
    p.voxel_res = 2.0 * res
    ctx.chk(L.rgc_set_params(h, C.byref(p)))
    ctx.chk(L.rgc_set_source(h, _DUMMY_SCAN.ctypes.data, len(_DUMMY_SCAN), 12))
    ctx.chk(L.rgc_clear_source(h))
    p.voxel_res = res
    ctx.chk(L.rgc_set_params(h, C.byref(p)))
    ctx.chk(L.rgc_set_neighbor_search(h, method, float(radius)))
    ctx.chk(L.rgc_set_regularization_method(h, reg))
    ctx.chk(L.rgc_set_voxel_accumulation_mode(h, 0))
    ctx.chk(L.rgc_set_rbf_kernel(h, float(rbf[0]), float(rbf[1])))
    ctx.chk(L.rgc_set_covariance_estimation(h, cov))
    ctx.chk(L.rgc_set_target_lazy(h, 0))


def set_clouds(ctx, o, inp, form, tgt="tgt", src="src"):
    """the clouds of a registration object `o` (a view of the context), in either form; the device inputs stay alive with the clouds"""
    if form == "host":
        o.setInputTarget(inp[tgt])
        o.setInputSource(inp[src])
        ctx.hold("reg", [])
        return
    dt, ds = Dev(ctx, inp[tgt]), Dev(ctx, inp[src])          # both uploads are enqueued before rgc_set_target*: the source may be handed over unsynchronised
    o.setInputTargetDevice(dt.addr, len(dt), dt.stride_bytes)
    o.setInputSourceDevice(ds.addr, len(ds), ds.stride_bytes)
    ctx.hold("reg", [dt, ds])


def _solve_out(o, aligned=None, fitness=None):
    out = dict(T=o.getFinalTransformation(), H=o.getFinalHessian(), iterations=int(o.nr_iterations), converged=bool(o.hasConverged()), lm_failed=bool(o.lm_failed))
    if aligned is not None:
        out["aligned"] = aligned
    if fitness is not None:
        out["fitness"] = float(fitness)
    return out


def kept_reg(name, frozen=None, source=True):
    """the clouds' covariances and the voxel map (sorted by voxel: the dump is 'unordered'), and the frozen cost of the method that linearised last"""
    def kept(ctx):
        o = ctx.view(name)
        out = dict(target_cov=o.getTargetCovariances(), voxels=o.getVoxels())
        if source:
            out["source_cov"] = o.getSourceCovariances()
        if frozen is not None:
            out["frozen"] = frozen(ctx, o)
        return out
    return kept


def _vgicp_align(method, radius=-1.0, reg=REG_PLANE, cov=0, rbf=(0.5, 3.0)):
    def run(ctx, inp, form):
        v = ctx.view("vgicp")
        route(ctx, method, radius, reg, cov, rbf)
        set_clouds(ctx, v, inp, form)
        aligned = v.align(inp["guess"], want_output=True, want_fitness=True)
        return _solve_out(v, aligned, v.getFitnessScore())
    return run


def run_vgicp_halves(ctx, inp, form):
    v = ctx.view("vgicp")
    route(ctx)
    set_clouds(ctx, v, inp, form)
    v.align_begin(inp["guess"], want_fitness=True)
    v.align_end()
    out = _solve_out(v, fitness=v.getFitnessScore())
    d = Dev(ctx, np.zeros((len(inp["src"]), 4), np.float32))
    v.alignedToDevice(d.addr, 16)
    out["aligned_device"] = d.numpy()[:, :3].copy()
    d.free()
    out["fitness_at"] = float(v.fitnessAt(inp["T_b"]))
    return out


def _frozen_vgicp(ctx, o):
    return dict(cost=float(o.compute_error(reg_inputs("small")["T_b"])), n=int(o.num_correspondences))


def _vgicp_linearize(method, radius=-1.0):
    def run(ctx, inp, form):
        v = ctx.view("vgicp")
        route(ctx, method, radius)
        set_clouds(ctx, v, inp, form)
        cost, H, b = v.linearize(inp["T_a"])
        return dict(cost=float(cost), H=H, b=b, n=int(v.num_correspondences), error_b=float(v.compute_error(inp["T_b"])), cost_only=float(v.evaluateCost(inp["T_a"])))
    return run


def run_vgicp_getters(ctx, inp, form):
    v = ctx.view("vgicp")
    route(ctx)
    set_clouds(ctx, v, inp, form)
    out = dict(source_cov=v.getSourceCovariances(), target_cov=v.getTargetCovariances(), source_normals=np.abs(v.getSourceNormals()),
               target_normals=np.abs(v.getTargetNormals()), voxels=v.getVoxels())
    v.setSourceCovariances(out["source_cov"][::-1].copy())            # plane-form covariances of other points: representable, and not what was computed
    v.setTargetCovariances(out["target_cov"][::-1].copy())
    out["voxels_from_given"] = v.getVoxels()
    out["cost_from_given"] = float(v.linearize(inp["T_a"])[0])
    return out


def run_vgicp_swap_clear(ctx, inp, form):
    v = ctx.view("vgicp")
    route(ctx)
    set_clouds(ctx, v, inp, form)
    v.swapSourceAndTarget()
    out = dict(voxels_swapped=v.getVoxels(), source_cov=v.getSourceCovariances(), cost=float(v.linearize(np.linalg.inv(inp["T_a"]))[0]))
    v.clearSource()
    v.clearTarget()
    set_clouds(ctx, v, inp, form)
    v.clearSource()
    out["target_cov"] = v.getTargetCovariances()
    return out


def run_vgicp_resolution(ctx, inp, form):
    v = ctx.view("vgicp")
    route(ctx)
    set_clouds(ctx, v, inp, form)
    p = P()._lib.Params()
    ctx.chk(ctx.L.rgc_get_params(ctx.h, C.byref(p)))
    res = p.voxel_res
    out = dict(voxels_res=v.getVoxels()["coords"])
    try:
        p.voxel_res = 0.5
        ctx.chk(ctx.L.rgc_set_params(ctx.h, C.byref(p)))                 # "prepares the clouds the context holds again, from their inputs"
        out["voxels_half"] = v.getVoxels()
        v.align(inp["guess"], want_output=False)
        out.update(_solve_out(v))
    finally:
        p.voxel_res = res
        ctx.chk(ctx.L.rgc_set_params(ctx.h, C.byref(p)))
    return out


def run_vgicp_reframed(ctx, inp, form):
    """the re-framed target (always device memory), the solve in halves ended by rgc_align_end_reframe onto the same context"""
    v = ctx.view("vgicp")
    route(ctx)
    a = np.zeros((len(inp["tgt"]), 4), np.float32)
    a[:, :3] = inp["tgt"]
    d_map, d_body, ds = Dev(ctx, a), Dev(ctx, np.zeros_like(a)), Dev(ctx, inp["src"])
    v.setNeighbourReuse(v.REUSE_LISTS)
    q, t = np.array([0.0, 0.0, np.sin(0.004), np.cos(0.004)]), np.array([0.03, -0.02, 0.001])
    v.setInputTargetReframed(d_map.addr, len(a), 16, q, t, d_body.addr)
    v.setInputSourceDevice(ds.addr, len(ds), ds.stride_bytes)
    ctx.hold("reg", [d_map, d_body, ds])
    out = dict(body=d_body.numpy(), target_cov=v.getTargetCovariances())
    v.align_begin(inp["guess"], want_fitness=True)
    Tw = np.eye(4)
    v.align_end_reframe(v, Tw, d_map.addr, len(a), 16, d_body.addr)
    out.update(_solve_out(v, fitness=v.getFitnessScore()), world=Tw, body_next=d_body.numpy(), target_cov_next=v.getTargetCovariances())
    return out


def _gicp(name, reset=False):
    def run(ctx, inp, form):
        o = ctx.view(name)
        route(ctx)
        o.setMaxCorrespondenceDistance(1.5)
        set_clouds(ctx, o, inp, form)
        cost, H, b = o.linearize(inp["T_a"])
        out = dict(cost=float(cost), H=H, b=b, n=int(o.num_correspondences), error_b=float(o.compute_error(inp["T_b"])), corr=list(o.correspondences()))
        if reset:
            cost2, H2, b2 = o.linearize(inp["T_b"])                                     # the anchors of the first linearisation decide who is searched
            out.update(cost2=float(cost2), H2=H2, b2=b2, searched2=int(o.num_searched()), corr2=list(o.correspondences()))
            o.reset()
        aligned = o.align(inp["guess"], want_output=True, want_fitness=True)
        out.update(_solve_out(o, aligned, o.getFitnessScore()))
        out["cost_after"] = float(o.linearize(inp["T_a"], want_H=False)[0])
        return out
    return run


def _frozen_gicp(ctx, o):
    return dict(cost=float(o.compute_error(reg_inputs("small")["T_b"])), n=int(o.num_correspondences), corr=list(o.correspondences()))


def run_gicpmp(ctx, inp, form):
    o = ctx.view("gicpmp")
    route(ctx)
    o.setNeighborSearchRadius(0.5)
    o.setMaximumIterations(16)
    set_clouds(ctx, o, inp, form)
    cost, H, b = o.linearize(inp["T_a"])
    out = dict(cost=float(cost), H=H, b=b, n=int(o.num_correspondences), pairs=int(o.num_pairs), candidates=int(o.num_candidates), merged=list(o.merged()),
               neighbors=list(o.neighbors()))
    aligned = o.align(inp["guess"], want_output=True, want_fitness=True)
    out.update(_solve_out(o, aligned, o.getFitnessScore()))
    out["cost_after"] = float(o.linearize(inp["T_a"], want_H=False)[0])
    return out


def _frozen_gicpmp(ctx, o):
    return dict(n=int(o.num_correspondences), pairs=int(o.num_pairs), merged=list(o.merged()), neighbors=list(o.neighbors()))


# ---- NDT -----------------------------------------------------------------------------------------------------------------------------------------------------
def _ndt_voxels(o, which, raw=False):
    v = o.voxels(which, raw=raw)
    order = np.lexsort((v["coords"][:, 2], v["coords"][:, 1], v["coords"][:, 0]))
    return {k: a[order] for k, a in v.items()}


def _ndt_set(ctx, o, inp, form, tgt="tgt", src="src"):
    o.setResolution(1.0)
    if form == "host":
        o.setInputTarget(inp[tgt]); o.setInputSource(inp[src])
        ctx.hold("ndt", [])
    else:
        dt, ds = Dev(ctx, inp[tgt]), Dev(ctx, inp[src])
        o.setInputTarget(dt); o.setInputSource(ds)
        ctx.hold("ndt", [dt, ds])


def _ndt(mode):
    def run(ctx, inp, form):
        p, o = P(), ctx.view("ndt")
        o.setDistanceMode(mode)
        o.setNeighborSearchMethod(p.ndt.NDT_DIRECT7)
        _ndt_set(ctx, o, inp, form)
        cost, H, b = o.linearize(inp["T_a"])
        out = dict(cost=float(cost), H=H, b=b, n=int(o.num_correspondences()), error_b=float(o.compute_error(inp["T_b"])), target=_ndt_voxels(o, 0, raw=True))
        T = o.align(inp["guess"])
        out.update(T=T.copy(), H_final=o.getFinalHessian().copy(), iterations=int(o.iterations()), converged=bool(o.hasConverged()), lm_failed=bool(o.lmFailed()))
        out["cost_after"] = float(o.linearize(inp["T_a"], want_H=False)[0])
        return out
    return run


def kept_ndt(ctx):
    o = ctx.view("ndt")
    out = dict(params=o.getParams(), target=_ndt_voxels(o, 0), frozen_n=int(o.num_correspondences()), frozen_cost=float(o.compute_error(reg_inputs("small")["T_b"])))
    if out["params"]["distance_mode"] == P().ndt.NDT_D2D:    # (P2D has no voxel map of the source)
        out["source"] = _ndt_voxels(o, 1)
    return out


def run_ndt_swap_clear(ctx, inp, form):
    p, o = P(), ctx.view("ndt")
    o.setDistanceMode(p.ndt.NDT_D2D)
    o.setNeighborSearchMethod(p.ndt.NDT_DIRECT1)
    _ndt_set(ctx, o, inp, form)
    o.swapSourceAndTarget()
    out = dict(target=_ndt_voxels(o, 0), cost=float(o.linearize(np.linalg.inv(inp["T_a"]), want_H=False)[0]))
    o.clearSource(); o.clearTarget()
    _ndt_set(ctx, o, inp, form)
    out["cost_again"] = float(o.linearize(inp["T_a"], want_H=False)[0])
    return out


# ---- the features on a cloud of their own -----------------------------------------------------------------------------------------------------------------------
def _case_of(module, name):
    import importlib
    m = importlib.import_module(module)
    if hasattr(m, "case"):
        return m.case(name)
    cs = m.cases() if hasattr(m, "cases") else {c["name"]: c for c in m.all_cases()}
    return cs[name]


@functools.lru_cache(maxsize=None)
def _outlier_big():
    return _case_of("outlier_cases", "big")["cloud"]


@functools.lru_cache(maxsize=None)
def search_inputs(size):
    """small: search_cases 'lattice' (6457 points, 1660 queries; k = 32 at cell 1/16 takes the cube-growth path); large: outlier_cases 'big' (70001 points),
    its first 2000 points as queries"""
    if size == "small":
        c = _case_of("search_cases", "lattice")
        return dict(tgt=c["tgt"], qry=c["qry"], k=32, cell=0.0625, radius=0.125, max_nn=5)
    big = _outlier_big()
    return dict(tgt=big, qry=np.ascontiguousarray(big[:2000]), k=8, cell=0.0, radius=0.5, max_nn=5)


SEARCH_COVERS = {"rgc_search_set_cloud", "rgc_search_clear", "rgc_search_get_info"}


def run_search_knn(ctx, inp, form):
    t, bufs = ctx.view("tree"), []
    t.clear()
    try:
        t.setInputCloud(up(ctx, form, inp["tgt"], bufs), cell=inp["cell"])
        idx, sq = t.nearestKSearch(up(ctx, form, inp["qry"], bufs), inp["k"])
    except Exception:
        free(bufs)
        raise
    ctx.hold("search", bufs)
    return dict(idx=idx, sq=sq, info=t.info())


def run_search_radius(ctx, inp, form):
    t, bufs = ctx.view("tree"), []
    try:
        t.setInputCloud(up(ctx, form, inp["tgt"], bufs), cell=inp["cell"])
        q = up(ctx, form, inp["qry"], bufs)
        out = dict(all=list(t.radiusSearch(q, inp["radius"], 0, True)), info_all=t.info(), nearest=list(t.radiusSearch(q, inp["radius"], inp["max_nn"], True)), info=t.info())
    except Exception:
        free(bufs)
        raise
    ctx.hold("search", bufs)
    return out


def kept_search(ctx):
    """the index's answers to fixed queries (host queries, k = 5) and the record of that query call"""
    t = ctx.view("tree")
    idx, sq = t.nearestKSearch(_case_of("search_cases", "lattice")["qry"][:200], 5)
    return dict(idx=idx, sq=sq, info=t.info())


def _filter(view, module, names, setup, result, cloud_key="cloud"):
    def make(size):
        return dict(_case_of(module, names[size]))

    def run(ctx, inp, form):
        o, bufs = ctx.view(view), []
        setup(o, inp)
        o.setInputCloud(up(ctx, form, inp[cloud_key], bufs))
        try:
            return result(o)
        finally:
            free(bufs)
    return make, run


def _info(view):
    return lambda ctx: dict(info=ctx.view(view).info())


def _sor_setup(o, c):
    o.setMeanK(c["sor"][0][0]); o.setStddevMulThresh(c["sor"][0][1]); o.setNegative(False)


def _ror_setup(o, c):
    o.setRadiusSearch(c["ror"][0][0]); o.setMinNeighborsInRadius(c["ror"][0][1]); o.setNegative(False)


def _cluster_setup(o, c):
    o.setClusterTolerance(c["tol"][0]); o.setMinClusterSize(c["limits"][0][0]); o.setMaxClusterSize(c["limits"][0][1])


def _plane_setup(o, c):
    o._init_params()
    prm = c["prm"]
    o.setDistanceThreshold(prm["threshold"]); o.setMaxIterations(prm["max_iterations"]); o.setProbability(prm["probability"])
    o.setOptimizeCoefficients(bool(prm["optimize"])); o.setSeed(prm["seed"]); o.setSamples(c["samples"])


def _plane_result(o):
    idx, coeff = o.segment(with_counts=True)
    return dict(idx=idx, coeff=coeff, counts=o.counts(), info=o.info(), inliers=o.filter())


def _normal_make(names):
    def make(size):
        module, name, sub, k, radius = names[size]
        c = _case_of(module, name)
        if sub is None:
            cloud, surface = c["cloud"], c.get("surface")
        else:                                                # the first `sub` points of a designed cloud as queries over the whole of it as the surface
            cloud, surface = np.ascontiguousarray(c["cloud"][:sub]), c["cloud"]
        return dict(cloud=cloud, surface=surface, k=k, radius=radius)
    return make


def run_normals(ctx, inp, form):
    o, bufs = ctx.view("normal"), []
    o._init_params()
    o.setInputCloud(up(ctx, form, inp["cloud"], bufs))
    if inp["surface"] is not None:
        o.setSearchSurface(up(ctx, form, inp["surface"], bufs))
    if inp["k"]:
        o.setKSearch(inp["k"])
    else:
        o.setRadiusSearch(inp["radius"])
    o.setViewPoint(0.2, -0.3, 5.0)
    try:
        n = o.compute(with_moments=True)
        return dict(normals=n, cov=o.getCovariances(), centroids=o.getCentroids(), counts=o.getCounts(), n_valid=int(o.getValidCount()), info=o.info())
    finally:
        free(bufs)


def _fpfh_make(names):
    def make(size):
        name, sub = names[size]
        c = _case_of("fpfh_cases", name)
        if sub is None:
            return dict(cloud=c["cloud"], surface=c["surface"], normals=c["normals"], radius=c["radius"])
        return dict(cloud=np.ascontiguousarray(c["cloud"][:sub]), surface=c["cloud"], normals=c["normals"], radius=c["radius"])
    return make


def run_fpfh(ctx, inp, form):
    o, bufs = ctx.view("fpfh"), []
    o._init_params()
    o.setInputCloud(up(ctx, form, inp["cloud"], bufs))
    if inp["surface"] is not None:
        o.setSearchSurface(up(ctx, form, inp["surface"], bufs))
    o.setInputNormals(up(ctx, form, inp["normals"], bufs))
    o.setRadiusSearch(inp["radius"])
    try:
        f = o.compute(with_spfh=True)
        spfh, scnt = o.getSPFH()
        return dict(fpfh=f, spfh=spfh, spfh_counts=scnt, counts=o.getCounts(), n_valid=int(o.getValidCount()), info=o.info())
    finally:
        free(bufs)


# ---- the stages of the frame body: leaf filter, uniform sampling, de-skew, re-framing, front-end, wire -----------------------------------------------------------------
def _vg_route(ctx):
    """of rgc_voxelgrid_route the fields that do not depend on the context's history (the path, the kept box and the chain's shape do, by design: 'a context
    remembers the leaf box of the last cloud per leaf size'; 'the filter's OUTPUT never depends on the route')"""
    r = ctx.view("pre").voxelGridRoute()
    return dict(route={k: r[k] for k in ("status", "n", "n_out")})


def _pre_call(ctx, fn, a, form, out_cols=4, extra=(), n_out=True, out_index=False):
    """one of the rgc_voxelgrid / rgc_uniform_sampling calls in either form: -> (records, indices or None)"""
    L, n, bufs = ctx.L, len(a), []
    src = up(ctx, form, a, bufs)
    cnt = C.c_int(0)
    try:
        if form == "host":
            out, idx = np.full((n, out_cols), np.nan, np.float32), np.full(n, -1, np.int32)
            args = [out.ctypes.data] + ([idx.ctypes.data] if out_index else [])
            ctx.chk(fn(ctx.h, src.ctypes.data, n, src.strides[0], *extra, *args, C.byref(cnt), 0))
            return out[:cnt.value].copy(), idx[:cnt.value].copy() if out_index else None
        d_out, d_idx = Dev(ctx, np.zeros((n, out_cols), np.float32)), Dev(ctx, np.zeros(n, np.int32), np.int32)
        bufs += [d_out, d_idx]
        args = [d_out.ptr] + ([d_idx.ptr] if out_index else [])
        ctx.chk(fn(ctx.h, src.ptr, n, src.stride_bytes, *extra, *args, C.byref(cnt), 1))
        return d_out.numpy()[:cnt.value].copy(), d_idx.numpy()[:cnt.value].copy() if out_index else None
    finally:
        free(bufs)


def run_voxelgrid(ctx, inp, form):
    out, _ = _pre_call(ctx, ctx.L.rgc_voxelgrid, inp["xyzi"], form, extra=(C.c_float(0.3),))
    return dict(out=out, **_vg_route(ctx))


def vg_begin(ctx, inp):
    """rgc_voxelgrid_begin on an uploaded sweep; the pending halves are remembered on the context"""
    a = inp["xyzi"]
    d_in, d_out = Dev(ctx, a), Dev(ctx, np.zeros((len(a), 4), np.float32))
    rc = ctx.L.rgc_voxelgrid_begin(ctx.h, d_in.ptr, len(a), 16, C.c_float(0.3), d_out.ptr)
    if rc:
        d_in.free(); d_out.free()
        ctx.chk(rc)
    ctx.vg_open = (d_in, d_out)


def vg_end(ctx):
    d_in, d_out = ctx.vg_open
    ctx.vg_open = None
    n = C.c_int(0)
    try:
        ctx.chk(ctx.L.rgc_voxelgrid_end(ctx.h, C.byref(n)))
        return dict(out=d_out.numpy()[:n.value].copy(), **_vg_route(ctx))
    finally:
        d_in.free(); d_out.free()


def run_voxelgrid_halves(ctx, inp, form):
    vg_begin(ctx, inp)
    return vg_end(ctx)


@functools.lru_cache(maxsize=None)
def us_inputs(size):
    """small: us_cases.lattice() (3000 points on k / 16: exact ties at leaf 0.5); large: us_cases.big_leaves(64) (25395 points)"""
    import us_cases
    a = us_cases.lattice() if size == "small" else us_cases.big_leaves(64)[0]
    return dict(xyzc=np.ascontiguousarray(a, np.float32))


def run_uniform_sampling(ctx, inp, form):
    out, idx = _pre_call(ctx, ctx.L.rgc_uniform_sampling, inp["xyzc"], form, extra=(C.c_float(0.5),), out_index=True)
    return dict(out=out, idx=idx, **_vg_route(ctx))


def run_deskew(ctx, inp, form):
    dp = C.POINTER(C.c_double)
    q, t = np.ascontiguousarray(inp["q_motion"], np.float64), np.ascontiguousarray(inp["t_motion"], np.float64)
    if form == "host":
        return dict(out=ctx.view("pre").adjustDistortion(inp["xyzi"], q, t))
    d = Dev(ctx, inp["xyzi"])
    try:
        ctx.chk(ctx.L.rgc_deskew(ctx.h, d.ptr, len(d), 16, q.ctypes.data_as(dp), t.ctypes.data_as(dp), 1))
        return dict(out=d.numpy())
    finally:
        d.free()


def run_transform(ctx, inp, form):
    if form == "host":
        return dict(out=ctx.view("pre").transformPointCloud(inp["xyzi"], inp["q"], inp["t"]))
    d, o = Dev(ctx, inp["xyzi"]), Dev(ctx, np.zeros_like(inp["xyzi"]))
    try:
        ctx.view("vgicp").transformCloudDevice(d.addr, len(d), 16, inp["q"], inp["t"], o.addr)
        return dict(out=o.numpy())
    finally:
        d.free(); o.free()


def run_frontend(ctx, inp, form):
    fe = ctx.view("fe")
    if form == "host":
        out = fe.laserCloudHandler(inp["raw"])
    else:
        d = Dev(ctx, inp["raw"])
        try:
            out = fe._run(d.ptr, len(d), 16, True, on_device=True)
        finally:
            d.free()
    dc, n = C.c_void_p(), C.c_int(0)
    ctx.chk(ctx.L.rgc_frontend_cloud_device(ctx.h, C.byref(dc), C.byref(n)))
    resident = np.empty((n.value, 4), np.float32)
    if n.value:
        ctx.chk(ctx.L.rgc_download(ctx.h, resident.ctypes.data, dc, resident.nbytes))
    return dict(out, resident=resident)


@functools.lru_cache(maxsize=None)
def wire_inputs(size):
    """a Velodyne-layout message of 1000 / 5000 points (fuzz_one_context.py's) and the records to pack"""
    n = {"small": 1000, "large": 5000}[size]
    rng = np.random.default_rng(4600 + n)
    dt = np.dtype({"names": ["x", "y", "z", "intensity", "ring"], "formats": ["<f4", "<f4", "<f4", "<f4", "<u2"], "offsets": [0, 4, 8, 16, 20], "itemsize": 32})
    a = np.zeros(n, dt)
    for k in ("x", "y", "z", "intensity"):
        a[k] = rng.normal(0, 20, n).astype(np.float32)
    a["ring"] = rng.integers(0, 16, n)
    return dict(data=a.tobytes(), n=n, pts=np.stack([a["x"], a["y"], a["z"], a["intensity"]], axis=1), pts5=rng.normal(0, 5, (n, 5)).astype(np.float32))


def run_wire(ctx, inp, form):
    p, w = P(), ctx.view("wire")
    lay = p.wire.layout(32, dict(x=(0, 7), y=(4, 7), z=(8, 7), intensity=(16, 7), ring=(20, 4)))
    n = inp["n"]
    if form == "host":
        xyzi, ring, _ = w.unpack(inp["data"], n, lay, want_ring=True)
        return dict(xyzi=xyzi, ring=ring, packed=np.frombuffer(w.pack(inp["pts"]), np.uint8), packed5=np.frombuffer(w.pack(inp["pts5"], "xyzinormal"), np.uint8))
    buf = np.frombuffer(inp["data"], np.uint8)
    d_x, d_r, d_p = Dev(ctx, np.zeros((n, 4), np.float32)), Dev(ctx, np.zeros(n, np.int32), np.int32), Dev(ctx, inp["pts"])
    try:
        ctx.chk(ctx.L.rgc_pc2_unpack(ctx.h, buf.ctypes.data, n, C.byref(lay), d_x.ptr, d_r.ptr, None, 1))
        out, out5 = np.empty(n * 32, np.uint8), np.empty(n * 48, np.uint8)
        ctx.chk(ctx.L.rgc_pc2_pack(ctx.h, 0, d_p.ptr, n, 1, out.ctypes.data))
        d5 = Dev(ctx, inp["pts5"])
        try:
            ctx.chk(ctx.L.rgc_pc2_pack(ctx.h, 1, d5.ptr, n, 1, out5.ctypes.data))
        finally:
            d5.free()
        return dict(xyzi=d_x.numpy(), ring=d_r.numpy(), packed=out, packed5=out5)
    finally:
        d_x.free(); d_r.free(); d_p.free()


# ---- the keyframe store, the pose graph, the resident map, ICP, mapping registration ---------------------------------------------------------------------------------
def _kf_info(s):
    i = s.info()
    i.pop("revision")                                       # (a counter of the context's life)
    return i


def _kf_fill(ctx, inp):
    s = ctx.view("store")
    s.reset()
    for i, pose, c in zip(inp["ids"], inp["poses"], inp["clouds"]):
        s.push(int(i), pose, *c)
    return s


def run_kf_push_assemble(ctx, inp, form):
    s = _kf_fill(ctx, inp)
    out = dict(info=_kf_info(s), travel=list(s.travel(inp["ids"])))
    ids = inp["ids"][[4, 1, 7, 1]]
    if form == "host":
        out["plain"] = s.assemble(ids, (0, 1, 2)).copy()
        out["leaf"] = s.assemble(inp["ids"], (2,), leaf=0.4).copy()
    else:
        for key, sel, kinds, leaf in (("plain", ids, (0, 1, 2), 0.0), ("leaf", inp["ids"], (2,), 0.4)):
            dc = s.assemble(sel, kinds, leaf=leaf, device=True)
            try:
                out[key] = dc.numpy()
            finally:
                dc.close()                                  # (its __del__ would free it through the context: only while that is alive)
    s.set_poses(inp["moved_ids"], inp["moved"])
    out["info_moved"] = _kf_info(s)
    out["moved"] = s.assemble(inp["moved_ids"], (1,)).copy()
    return out


def kept_kf(ctx):
    s = ctx.view("store")
    ids = drive_inputs("small")["ids"]
    return dict(info=_kf_info(s), travel=list(s.travel(ids)), assemble=s.assemble(ids[:3], (0, 1)).copy())


def run_kf_select(ctx, inp, form):
    s = _kf_fill(ctx, inp)
    sur, n_in = s.select_surrounding(inp["poses"][-1, :3], radius=1.5, density=0.2, return_count=True)
    loop = s.detect_loop(history_search_radius=1.0, history_search_num=2, min_key_id=0)
    return dict(surrounding=sur, n_in=int(n_in), everything=s.select_global(0.3), loop=loop, info=_kf_info(s))


@functools.lru_cache(maxsize=None)
def pgo_inputs(size):
    """small: pgo_cases 'one_loop' (40 nodes); large: 'big_100_on_300' (300 nodes, 100 loops)"""
    import pgo_cases
    c = pgo_cases.cases()[{"small": "one_loop", "large": "big_100_on_300"}[size]]
    return dict(store_ids=list(c["store_ids"]), store_poses=c["store_poses"], ids=np.array(c["ids"], np.int32), loops=c["loops"])


def run_pgo(ctx, inp, form):
    import us_cases
    p, s = P(), ctx.view("store")
    s.reset()
    for i, pose in zip(inp["store_ids"], inp["store_poses"]):
        s.push(int(i), pose, us_cases.tiny_cloud(i), None, None)
    g = p.pose_graph.PoseGraph4DoF(s)
    g.loops = [p._lib.PgoLoop(L["key_curr"], L["key_loop"], (C.c_double * 3)(*[float(v) for v in L["t"]]), float(L["yaw"]), float(L["pitch"]), float(L["roll"]))
               for L in inp["loops"]]
    lin = g.linearize(inp["ids"], radius=1e4)
    rep, poses = g.optimize(inp["ids"], apply=True)
    return dict(linearize=lin, report=rep, poses=poses, info=_kf_info(s), assembled=s.assemble(inp["ids"][:5], (0,)).copy())


def kept_pgo(ctx):
    s = ctx.view("store")
    ids = pgo_inputs("small")["ids"]
    return dict(info=_kf_info(s), travel=list(s.travel(ids[:8])), assemble=s.assemble(ids[:8], (0,)).copy())


@functools.lru_cache(maxsize=None)
def map_inputs(size):
    """three sweeps of a short drive as the map's keyframes (synth; 150 / 700 azimuth steps), their poses, and a scan to register"""
    s = P().synth
    n_az = {"small": 150, "large": 700}[size]
    frames = []
    for j in range(3):
        T = s.se3(s.rot_zyx(0.05 * j, 0.0, 0.0), [0.4 * j, 0.1 * j, 0.0])
        sc = s.make_scan(_world(), T, n_az=n_az, seed=4700 + j)
        frames.append((np.concatenate([sc["xyz"], sc["intensity"][:, None]], axis=1).astype(np.float32), _quat(T[:3, :3]), T[:3, 3].copy()))
    return dict(frames=frames, src=np.ascontiguousarray(frames[2][0][::4, :3]), guess=np.eye(4, dtype=np.float32))


def _map_fill(ctx, inp):
    m = ctx.view("map")
    m.reset([0.5, -0.5, 0.0])
    return m, [m.insert(a, q, t) for a, q, t in inp["frames"]]


def run_map_edit(ctx, inp, form):
    m, ids = _map_fill(ctx, inp)
    out = dict(n=len(ids), info=m.info(), points=m.points())
    out["evicted"] = m.evict(max_keyframes=2)
    m.rebase([1.0, 0.25, 0.0])
    out.update(info_after=m.info(), points_after=m.points())
    return out


def _map_info(m):
    i = m.info()
    i.pop("revision"); i.pop("oldest_id"); i.pop("newest_id")       # (counters of the context's life: a keyframe id is never given twice)
    return i


def _drop_map_counters(r):
    for k in ("info", "info_after"):
        if k in r:
            for c in ("revision", "oldest_id", "newest_id"):
                r[k].pop(c, None)
    return r


def kept_map(ctx):
    m = ctx.view("map")
    return dict(info=_map_info(m), points=m.points())


def run_map_commit(ctx, inp, form):
    v = ctx.view("vgicp")
    route(ctx)
    m, _ = _map_fill(ctx, inp)
    n = m.commit(0.3)
    v.setInputSource(inp["src"])
    ctx.hold("reg", [])                                     # (after both clouds have been replaced)
    out = dict(n_target=int(n), target=m.target(), n_again=int(m.commit(0.3)), target_cov=v.getTargetCovariances(), info=m.info())
    v.align(inp["guess"], want_output=False, want_fitness=True)
    out.update(_solve_out(v, fitness=v.getFitnessScore()))
    return out


def kept_map_commit(ctx):
    m, v = ctx.view("map"), ctx.view("vgicp")
    return dict(info=_map_info(m), points=m.points(), target=m.target(), target_cov=v.getTargetCovariances(), voxels=v.getVoxels())


ICP_N = {"small": (4000, 800), "large": (16000, 3200)}


@functools.lru_cache(maxsize=None)
def icp_inputs(size):
    """tests/test_icp.py's clouds (a synth map and a scan of it) at a fifteenth and a quarter of their size, as x, y, z, c records"""
    s = P().synth
    nt, ns = ICP_N[size]
    world, tgt = s.make_world_and_map(nt, seed=4800)
    src = s.make_scan_n(world, s.se3(s.rot_zyx(0.01, 0.0, 0.0), [0.08, -0.03, 0.0]), ns, seed=4801)["xyz"]
    pad = lambda a: np.ascontiguousarray(np.concatenate([a, np.zeros((len(a), 1))], axis=1), np.float32)   # noqa: E731
    return _ro(dict(tgt=pad(tgt), src=pad(src)))


def run_icp(ctx, inp, form):
    o, bufs = ctx.view("icp"), []
    o.setInputSource(up(ctx, form, inp["src"], bufs))
    o.setInputTarget(up(ctx, form, inp["tgt"], bufs))
    try:
        T = o.align()
        return dict(T=T.copy(), fitness=float(o.getFitnessScore()), converged=bool(o.hasConverged()), iterations=int(o.nr_iterations), state=o.convergence_state)
    finally:
        free(bufs)


@functools.lru_cache(maxsize=None)
def mapreg_inputs(size):
    """mapreg_cases: its maps, and the features of 'lm_rejected_cap' (124) / 'lm_function' (880)"""
    import mapreg_cases as mc
    c = mc.build({"small": "lm_rejected_cap", "large": "lm_function"}[size])
    corner, surf = mc.maps()
    pad = lambda a: np.ascontiguousarray(a if a.shape[1] == 4 else np.concatenate([a, np.zeros((len(a), 1))], axis=1), np.float32)   # noqa: E731
    return dict(corner=pad(np.asarray(corner, np.float32)), surf=pad(np.asarray(surf, np.float32)), feat=c["feat"], x0=c["x0"], x_eval=c["x_eval"], ground=c["ground"],
                imu=c["imu"])


def run_mapreg(ctx, inp, form):
    r, bufs = ctx.view("mapreg"), []
    try:
        r.setInputMaps(up(ctx, form, inp["corner"], bufs), up(ctx, form, inp["surf"], bufs))
    except Exception:
        free(bufs)
        raise
    ctx.hold("mapreg", bufs)
    f, x0 = inp["feat"], inp["x0"]
    out = dict(edge=r.associate(f[0], x0[0:4], x0[4:7], "edge"), plane=r.associate(f[1], x0[0:4], x0[4:7], "plane"))
    out["linearize"] = r.linearize(f[0], f[1], f[2], f[3], x0, inp["x_eval"], ground_cur=inp["ground"][0], ground_last=inp["ground"][1], imu=inp["imu"], want_factors=True)
    q1, t1, q2, t2, rep = r.optimize(f[0], f[1], f[2], f[3], x0[0:4], x0[4:7], x0[7:11], x0[11:14], ground_cur=inp["ground"][0], ground_last=inp["ground"][1], imu=inp["imu"])
    out.update(q_curr=q1, t_curr=t1, q_last=q2, t_last=t2, report=rep)
    return out


def kept_mapreg(ctx):
    c = mapreg_inputs("small")
    return dict(plane=ctx.view("mapreg").associate(c["feat"][1], c["x0"][0:4], c["x0"][4:7], "plane"))


# ---- the table --------------------------------------------------------------------------------------------------------------------------------------------------
class Op:
    def __init__(self, name, covers, sizes, make, run, kept=None, reads=(), writes=(), in_flight="refused", forms=("host", "device"), begin=None, end=None,
                 refused_whole=True, post=None):
        self.name, self.covers, self.sizes, self.make, self._run, self._kept = name, set(covers), dict(sizes), make, run, kept
        self.reads, self.writes, self.in_flight, self.forms = set(reads), set(writes) | set(reads), in_flight, tuple(forms)
        self.begin, self.end = begin, end                   # an operation that can be left open across the next ones (the leaf filter's halves)
        self.refused_whole = refused_whole                  # False: calls of the operation's own store run before the refused one (rgc_map_commit)
        self._post = post

    def run(self, ctx, size, form):
        ctx.history.append("%s[%s,%s]" % (self.name, size, form))
        out = self._run(ctx, self.make(size), form)
        return self._post(out) if self._post else out

    def kept(self, ctx):
        return self._kept(ctx) if self._kept else {}


_REG = ROUTE_COVERS | CLOUD_COVERS
_reg_sizes = {"small": "synth map 5000 / scan 1250 (the fuzz scripts' size)", "large": "synth map 20000 / scan 5000 (smoke()'s)"}
_scan_sizes = {"small": "synth sweep, 16 rings x 300 azimuth steps", "large": "synth sweep, 16 rings x 1500 azimuth steps"}
_feature_sizes = lambda m, a, b: {"small": "%s '%s'" % (m, a), "large": "%s '%s'" % (m, b)}   # noqa: E731

_sor = _filter("sor", "outlier_cases", {"small": "n_257", "large": "n_2049"}, _sor_setup,
               lambda o: dict(kept=o.filter(with_mean_distances=True), idx=o.getIndices(), mean_dist=o.getMeanDistances(), info=o.info()))
_ror = _filter("ror", "outlier_cases", {"small": "n_257", "large": "n_2049"}, _ror_setup,
               lambda o: dict(kept=o.filter(with_counts=True), idx=o.getIndices(), counts=o.getCounts(), info=o.info()))
_clu = _filter("cluster", "cluster_cases", {"small": "helix_257_shuf", "large": "helix_4097_shuf"}, _cluster_setup,
               lambda o: dict(clusters=[c.copy() for c in o.extract()][:50], labels=o.labels(), offsets=o.offsets(), indices=o.indices(), info=o.info()))
_pla = _filter("plane", "plane_cases", {"small": "size_257", "large": "size_65535"}, _plane_setup, _plane_result)

OPS = {o.name: o for o in [
    Op("vgicp_direct1", _REG | {"rgc_align", "rgc_get_aligned"}, _reg_sizes, reg_inputs, _vgicp_align(DIRECT1), kept_reg("vgicp"), reads=["reg"]),
    Op("vgicp_direct7", _REG | {"rgc_align", "rgc_get_aligned"}, _reg_sizes, reg_inputs, _vgicp_align(DIRECT7), kept_reg("vgicp"), reads=["reg"]),
    Op("vgicp_direct27", _REG | {"rgc_align", "rgc_get_aligned"}, _reg_sizes, reg_inputs, _vgicp_align(DIRECT27), kept_reg("vgicp"), reads=["reg"]),
    Op("vgicp_radius", _REG | {"rgc_align", "rgc_get_aligned"}, _reg_sizes, reg_inputs, _vgicp_align(DIRECT_RADIUS, 1.5), kept_reg("vgicp"), reads=["reg"]),
    Op("vgicp_general_route", _REG | {"rgc_align", "rgc_get_aligned"}, _reg_sizes, reg_inputs, _vgicp_align(DIRECT1, reg=REG_MIN_EIG), kept_reg("vgicp"), reads=["reg"]),
    Op("vgicp_rbf_covariances", _REG | {"rgc_align", "rgc_get_aligned"}, _reg_sizes, reg_inputs, _vgicp_align(DIRECT1, cov=1, rbf=(2.0, 0.6)), kept_reg("vgicp"), reads=["reg"]),
    Op("vgicp_align_in_halves", _REG | {"rgc_align_begin", "rgc_align_end", "rgc_get_aligned_device", "rgc_fitness"}, _reg_sizes, reg_inputs, run_vgicp_halves,
       kept_reg("vgicp"), reads=["reg"]),
    Op("vgicp_linearize_direct7", _REG | {"rgc_linearize", "rgc_compute_error", "rgc_num_correspondences"}, _reg_sizes, reg_inputs, _vgicp_linearize(DIRECT7),
       kept_reg("vgicp", _frozen_vgicp), reads=["reg"]),
    Op("vgicp_linearize_radius", _REG | {"rgc_linearize", "rgc_compute_error", "rgc_num_correspondences"}, _reg_sizes, reg_inputs, _vgicp_linearize(DIRECT_RADIUS, 2.0),
       kept_reg("vgicp", _frozen_vgicp), reads=["reg"]),
    Op("vgicp_getters", _REG | {"rgc_get_source_covariances", "rgc_get_target_covariances", "rgc_get_voxels", "rgc_set_source_covariances", "rgc_set_target_covariances",
                                "rgc_linearize"}, _reg_sizes, reg_inputs, run_vgicp_getters, kept_reg("vgicp"), reads=["reg"]),
    Op("vgicp_swap_clear", _REG | {"rgc_swap_source_and_target", "rgc_clear_source", "rgc_clear_target", "rgc_linearize", "rgc_get_voxels", "rgc_get_source_covariances",
                                   "rgc_get_target_covariances"}, _reg_sizes, reg_inputs, run_vgicp_swap_clear, kept_reg("vgicp", source=False), reads=["reg"]),
    Op("vgicp_new_resolution", _REG | {"rgc_set_params", "rgc_get_params", "rgc_align", "rgc_get_voxels"}, _reg_sizes, reg_inputs, run_vgicp_resolution, kept_reg("vgicp"),
       reads=["reg"]),
    Op("vgicp_reframed_target", ROUTE_COVERS | {"rgc_set_target_reframed", "rgc_set_source_device", "rgc_set_knn_reuse", "rgc_align_begin", "rgc_align_end_reframe",
                                                "rgc_get_target_covariances"}, _reg_sizes, reg_inputs, run_vgicp_reframed, kept_reg("vgicp"), reads=["reg"],
       forms=("device",)),
    Op("fast_gicp", _REG | {"rgc_gicp_set_max_correspondence_distance", "rgc_gicp_linearize", "rgc_gicp_compute_error", "rgc_gicp_num_correspondences",
                            "rgc_gicp_get_correspondences", "rgc_gicp_align", "rgc_get_aligned"}, _reg_sizes, reg_inputs, _gicp("gicp"),
       kept_reg("gicp", _frozen_gicp), reads=["reg"]),
    Op("fast_gicp_single_thread", _REG | {"rgc_gicp_set_max_correspondence_distance", "rgc_gicpst_linearize", "rgc_gicpst_compute_error", "rgc_gicpst_num_correspondences",
                                          "rgc_gicpst_num_searched", "rgc_gicpst_get_correspondences", "rgc_gicpst_reset", "rgc_gicpst_align", "rgc_get_aligned"}, _reg_sizes, reg_inputs, _gicp("gicpst", reset=True),
       kept_reg("gicpst", _frozen_gicp), reads=["reg"]),
    Op("fast_gicp_multi_points", _REG | {"rgc_gicpmp_set_params", "rgc_gicpmp_linearize", "rgc_gicpmp_num_correspondences", "rgc_gicpmp_num_candidates",
                                         "rgc_gicpmp_get_merged", "rgc_gicpmp_get_neighbors", "rgc_gicpmp_align", "rgc_get_aligned"}, _reg_sizes,
       reg_inputs, run_gicpmp, kept_reg("gicpmp", _frozen_gicpmp), reads=["reg"]),
    Op("ndt_p2d", {"rgc_ndt_set_params", "rgc_ndt_set_target", "rgc_ndt_set_source", "rgc_ndt_set_target_device", "rgc_ndt_set_source_device", "rgc_ndt_linearize",
                   "rgc_ndt_compute_error", "rgc_ndt_num_correspondences", "rgc_ndt_align", "rgc_ndt_get_voxels", "rgc_ndt_get_raw_covariances"}, _reg_sizes, reg_inputs,
       _ndt(0), kept_ndt, reads=["ndt"], in_flight="runs"),
    Op("ndt_d2d", {"rgc_ndt_set_params", "rgc_ndt_set_target", "rgc_ndt_set_source", "rgc_ndt_set_target_device", "rgc_ndt_set_source_device", "rgc_ndt_linearize",
                   "rgc_ndt_compute_error", "rgc_ndt_num_correspondences", "rgc_ndt_align", "rgc_ndt_get_voxels", "rgc_ndt_get_raw_covariances"}, _reg_sizes, reg_inputs,
       _ndt(1), kept_ndt, reads=["ndt"], in_flight="runs"),
    Op("ndt_swap_clear", {"rgc_ndt_set_params", "rgc_ndt_set_target", "rgc_ndt_set_source", "rgc_ndt_set_target_device", "rgc_ndt_set_source_device",
                          "rgc_ndt_swap_source_and_target", "rgc_ndt_clear_source", "rgc_ndt_clear_target", "rgc_ndt_linearize", "rgc_ndt_get_voxels"}, _reg_sizes,
       reg_inputs, run_ndt_swap_clear, kept_ndt, reads=["ndt"], in_flight="runs"),
    Op("search_knn", SEARCH_COVERS | {"rgc_search_knn"}, {"small": "search_cases 'lattice', k = 32 at cell 1/16 (cube growth)", "large": "outlier_cases 'big' (70001), k = 8"},
       search_inputs, run_search_knn, kept_search, reads=["search", "search_info"]),
    Op("search_radius", SEARCH_COVERS | {"rgc_search_radius"}, {"small": "search_cases 'lattice', r = 1/8", "large": "outlier_cases 'big' (70001), r = 0.5"},
       search_inputs, run_search_radius, kept_search, reads=["search", "search_info"]),
    Op("outlier_statistical", {"rgc_outlier_statistical", "rgc_outlier_get_info"}, _feature_sizes("outlier_cases", "n_257", "n_2049"), *_sor, _info("sor"),
       reads=["outlier_info"]),
    Op("outlier_radius", {"rgc_outlier_radius", "rgc_outlier_get_info"}, _feature_sizes("outlier_cases", "n_257", "n_2049"), *_ror, _info("ror"), reads=["outlier_info"]),
    Op("cluster_extract", {"rgc_cluster_extract", "rgc_cluster_get_info"}, _feature_sizes("cluster_cases", "helix_257_shuf", "helix_4097_shuf"), *_clu, _info("cluster"),
       reads=["cluster_info"]),
    Op("plane_segment", {"rgc_plane_segment", "rgc_plane_get_info"}, _feature_sizes("plane_cases", "size_257", "size_65535"), *_pla, _info("plane"), reads=["plane_info"]),
    Op("normals_k", {"rgc_normal_estimate", "rgc_normal_get_info"}, {"small": "normal_cases 'walls' (440), k = 6", "large": "normal_cases 'sparse' (2020), k = 10: cube growth"},
       _normal_make({"small": ("normal_cases", "walls", None, 6, 0.0), "large": ("normal_cases", "sparse", None, 10, 0.0)}), run_normals, _info("normal"), reads=["normal_info"]),
    Op("normals_radius", {"rgc_normal_estimate", "rgc_normal_get_info"}, {"small": "normal_cases 'walls' (440), r = 0.6", "large": "normal_cases 'sheet' (4000), r = 0.15"},
       _normal_make({"small": ("normal_cases", "walls", None, 0, 0.6), "large": ("normal_cases", "sheet", None, 0, 0.15)}), run_normals, _info("normal"), reads=["normal_info"]),
    Op("normals_k_surface", {"rgc_normal_estimate", "rgc_normal_get_info"},
       {"small": "normal_cases 'surface' (847 queries on 4000), k = 10", "large": "fpfh_cases 'big': its first 4096 points on all 20000, k = 10"},
       _normal_make({"small": ("normal_cases", "surface", None, 10, 0.0), "large": ("fpfh_cases", "big", 4096, 10, 0.0)}), run_normals, _info("normal"), reads=["normal_info"]),
    Op("normals_radius_surface", {"rgc_normal_estimate", "rgc_normal_get_info"},
       {"small": "normal_cases 'surface' (847 queries on 4000), r = 0.15", "large": "fpfh_cases 'big': its first 4096 points on all 20000, r = 0.15"},
       _normal_make({"small": ("normal_cases", "surface", None, 0, 0.15), "large": ("fpfh_cases", "big", 4096, 0, 0.15)}), run_normals, _info("normal"), reads=["normal_info"]),
    Op("fpfh", {"rgc_fpfh_estimate", "rgc_fpfh_get_info"}, _feature_sizes("fpfh_cases", "lattice_16", "sphere"), _fpfh_make({"small": ("lattice_16", None), "large": ("sphere", None)}),
       run_fpfh, _info("fpfh"), reads=["fpfh_info"]),
    Op("fpfh_surface", {"rgc_fpfh_estimate", "rgc_fpfh_get_info"}, {"small": "fpfh_cases 'keypoints' (64 queries on 4000)", "large": "fpfh_cases 'big': its first 1024 points on all 20000"},
       _fpfh_make({"small": ("keypoints", None), "large": ("big", 1024)}), run_fpfh, _info("fpfh"), reads=["fpfh_info"]),
    Op("voxelgrid", {"rgc_voxelgrid", "rgc_voxelgrid_route"}, _scan_sizes, scan_inputs, run_voxelgrid, _vg_route, reads=["vg_route"], in_flight="runs"),
    Op("voxelgrid_in_halves", {"rgc_voxelgrid_begin", "rgc_voxelgrid_end", "rgc_voxelgrid_route"}, _scan_sizes, scan_inputs, run_voxelgrid_halves, _vg_route, reads=["vg_route"],
       in_flight="runs", forms=("device",), begin=vg_begin, end=vg_end),
    Op("uniform_sampling", {"rgc_uniform_sampling", "rgc_voxelgrid_route"}, {"small": "us_cases.lattice() (3000)", "large": "us_cases.big_leaves(64) (25395)"}, us_inputs,
       run_uniform_sampling, _vg_route, reads=["vg_route"], in_flight="runs"),
    Op("deskew", {"rgc_deskew"}, _scan_sizes, scan_inputs, run_deskew, in_flight="runs"),
    Op("transform_cloud", {"rgc_transform_cloud"}, _scan_sizes, scan_inputs, run_transform, in_flight="runs"),
    Op("frontend", {"rgc_frontend", "rgc_frontend_device", "rgc_frontend_cloud_device"}, _scan_sizes, scan_inputs, run_frontend, in_flight="runs"),
    Op("wire", {"rgc_pc2_unpack", "rgc_pc2_pack"}, {"small": "a Velodyne-layout message of 1000 points", "large": "of 5000 points"}, wire_inputs, run_wire, in_flight="runs"),
    Op("kf_push_assemble", {"rgc_kf_reset", "rgc_kf_push", "rgc_kf_set_poses", "rgc_kf_get_info", "rgc_kf_get_travel", "rgc_kf_assemble"},
       {"small": "12 keyframes of 16 x 60 sweeps (synth) on us_cases.square_drive poses", "large": "12 keyframes of 16 x 260 sweeps"}, drive_inputs, run_kf_push_assemble,
       kept_kf, reads=["kf"], writes=["vg_route"], in_flight="runs"),
    Op("kf_select", {"rgc_kf_reset", "rgc_kf_push", "rgc_kf_get_info", "rgc_kf_select_surrounding", "rgc_kf_select_global", "rgc_kf_detect_loop"},
       {"small": "12 keyframes of 16 x 60 sweeps (synth) on us_cases.square_drive poses", "large": "12 keyframes of 16 x 260 sweeps"}, drive_inputs, run_kf_select, kept_kf,
       reads=["kf"], writes=["vg_route"], in_flight="runs", forms=("host",)),
    Op("pose_graph", {"rgc_kf_reset", "rgc_kf_push", "rgc_kf_get_info", "rgc_kf_assemble", "rgc_pgo_linearize", "rgc_pgo_optimize"},
       _feature_sizes("pgo_cases", "one_loop", "big_100_on_300"), pgo_inputs, run_pgo, kept_pgo, reads=["kf"], in_flight="runs", forms=("host",)),
    Op("map_insert_evict_rebase", {"rgc_map_reset", "rgc_map_insert", "rgc_map_evict", "rgc_map_rebase", "rgc_map_get_info", "rgc_map_download"},
       {"small": "3 keyframes of 16 x 150 sweeps (synth)", "large": "3 keyframes of 16 x 700 sweeps"}, map_inputs, run_map_edit, kept_map, reads=["map"], in_flight="runs",
       forms=("host",), post=_drop_map_counters),
    Op("map_commit", ROUTE_COVERS | {"rgc_map_reset", "rgc_map_insert", "rgc_map_commit", "rgc_map_get_info", "rgc_map_download", "rgc_set_source", "rgc_align", "rgc_get_target_covariances"}, {"small": "3 keyframes of 16 x 150 sweeps (synth)", "large": "3 keyframes of 16 x 700 sweeps"}, map_inputs,
       run_map_commit, kept_map_commit, reads=["map", "reg"], writes=["vg_route"], forms=("host",), post=_drop_map_counters),
    Op("icp", {"rgc_icp_align", "rgc_icp_align_device"}, {"small": "synth map 4000 / scan 800 (tests/test_icp.py's clouds, smaller)", "large": "synth map 16000 / scan 3200"},
       icp_inputs, run_icp, in_flight="runs"),
    Op("mapping_registration", {"rgc_mapreg_set_maps", "rgc_mapreg_set_maps_device", "rgc_mapreg_associate", "rgc_mapreg_linearize", "rgc_mapreg_optimize"},
       {"small": "mapreg_cases 'lm_rejected_cap' (124 features)", "large": "mapreg_cases 'lm_function' (880 features); EXCEPTION to the four-times rule: both sizes "
        "register to the module's one pair of maps, so the map buffers do not grow -- the feature and factor buffers do"}, mapreg_inputs, run_mapreg, kept_mapreg, reads=["mapreg"], in_flight="runs"),
]}
OPS["map_commit"].refused_whole = False        # rgc_map_reset / rgc_map_insert run (route() selects nothing then), rgc_map_commit is what the solve in flight refuses


def points(inp):
    """the points an operation's inputs hold: every float32 array of more than 8 rows of 3 .. 6 columns (clouds, key poses), the clouds inside lists and tuples too, and a message's bytes"""
    n = 0
    for v in inp.values() if isinstance(inp, dict) else inp:
        if isinstance(v, np.ndarray) and v.dtype == np.float32 and v.ndim == 2 and 3 <= v.shape[1] <= 6 and len(v) > 8:
            n += len(v)
        elif isinstance(v, (list, tuple)):
            n += points(v)
        elif isinstance(v, (bytes, bytearray)):
            n += len(v) // 32
    return n


def drops(b, a):
    """does operation b replace what kept(a) reads?"""
    return bool(OPS[b].writes & OPS[a].reads)


# ---- running --------------------------------------------------------------------------------------------------------------------------------------------------
_lone = {}


def lone(name, size, form):
    """the operation on a fresh context of its own, computed once per (operation, size, form)"""
    key = (name, size, form)
    if key not in _lone:
        ctx = Ctx()
        try:
            _lone[key] = OPS[name].run(ctx, size, form)
        finally:
            ctx.close()
    return _lone[key]


def check(ctx, name, size, form, what="result"):
    """run on the shared context and compare with lone; an AssertionError carries the paths that differ and the history of calls"""
    got = OPS[name].run(ctx, size, form)
    bad = diff(got, lone(name, size, form))
    assert not bad, "%s[%s,%s] on the shared context differs from the same call on a context of its own at %s (%s)\nhistory: %s" % (
        name, size, form, ", ".join(bad[:8]), what, " -> ".join(ctx.history))
    return got


def check_kept(ctx, name, before, after_what):
    now = OPS[name].kept(ctx)
    bad = diff(now, before)
    assert not bad, "what %s left on the context changed at %s after %s\nhistory: %s" % (name, ", ".join(bad[:8]), after_what, " -> ".join(ctx.history))


def schedule(seed, n_ops, names=None):
    """a seeded schedule: (operation, size, form, leave a leaf filter open for this many operations, leave a solve in flight across the next operation)"""
    rng = np.random.default_rng(seed)
    names = sorted(OPS) if names is None else list(names)
    out = []
    for _ in range(n_ops):
        o = OPS[names[int(rng.integers(len(names)))]]
        out.append((o.name, SIZES[int(rng.integers(2))], o.forms[int(rng.integers(len(o.forms)))], int(rng.integers(1, 4)) if rng.random() < 0.15 else 0, rng.random() < 0.15))
    return out


def solve_begin(ctx, inp, reg=REG_PLANE):
    """a VGICP solve on the context's own clouds left in flight (lone_solve: the same solve undisturbed)"""
    v = ctx.view("vgicp")
    route(ctx, reg=reg)
    set_clouds(ctx, v, inp, "host")
    v.align_begin(inp["guess"], want_fitness=True)
    ctx.in_flight = True
    ctx.history.append("rgc_align_begin")


def solve_end(ctx):
    v = ctx.view("vgicp")
    v.align_end()
    ctx.in_flight = False
    ctx.history.append("rgc_align_end")
    return _solve_out(v, fitness=v.getFitnessScore())


def lone_solve(size="small", reg=REG_PLANE):
    key = ("solve", size, reg)
    if key not in _lone:
        ctx = Ctx()
        try:
            route(ctx, reg=reg)
            set_clouds(ctx, ctx.v, reg_inputs(size), "host")
            ctx.v.align_begin(reg_inputs(size)["guess"], want_fitness=True)
            _lone[key] = solve_end(ctx)
        finally:
            ctx.close()
    return _lone[key]


def run_schedule(ctx, sched):
    """every result against lone; a pending leaf filter and a solve in flight are ended where the schedule says; -> the number of comparisons"""
    compared, vg_left = 0, 0
    kept = {}
    inflight = False
    for name, size, form, leave_open, leave_solve in sched:
        o = OPS[name]
        if ctx.vg_open is not None:
            vg_left -= 1
            if vg_left <= 0 or name == "voxelgrid_in_halves":
                got = vg_end(ctx)
                bad = diff(got, lone("voxelgrid_in_halves", ctx.vg_size, "device"))
                assert not bad, "the leaf filter left open differs at %s\nhistory: %s" % (", ".join(bad[:8]), " -> ".join(ctx.history))
                compared += 1
                kept = {k: v for k, v in kept.items() if "vg_route" not in OPS[k].reads}
        if inflight and o.in_flight == "refused":
            assert same(solve_end(ctx), lone_solve()), "the solve left in flight differs\nhistory: %s" % " -> ".join(ctx.history)
            inflight = False
            compared += 1
            kept = {k: v for k, v in kept.items() if "reg" not in OPS[k].reads}
        if leave_open and name != "voxelgrid_in_halves" and ctx.vg_open is None:
            ctx.history.append("rgc_voxelgrid_begin[%s]" % size)
            vg_begin(ctx, scan_inputs(size))
            ctx.vg_size, vg_left = size, leave_open
        check(ctx, name, size, form)
        compared += 1
        kept = {k: v for k, v in kept.items() if not drops(name, k)}
        if o._kept:
            kept[name] = o.kept(ctx)
        if inflight:
            assert same(solve_end(ctx), lone_solve()), "the solve in flight across %s differs\nhistory: %s" % (name, " -> ".join(ctx.history))
            inflight = False
            compared += 1
            kept = {k: v for k, v in kept.items() if "reg" not in OPS[k].reads}
        elif leave_solve:
            solve_begin(ctx, reg_inputs("small"))
            inflight = True
            kept = {k: v for k, v in kept.items() if "reg" not in OPS[k].reads}
    if inflight:
        assert same(solve_end(ctx), lone_solve()), "the solve left in flight differs\nhistory: %s" % " -> ".join(ctx.history)
    if ctx.vg_open is not None:
        assert same(vg_end(ctx), lone("voxelgrid_in_halves", ctx.vg_size, "device")), "the leaf filter left open differs\nhistory: %s" % " -> ".join(ctx.history)
        kept = {k: v for k, v in kept.items() if "vg_route" not in OPS[k].reads}
    for k, before in kept.items():
        check_kept(ctx, k, before, "the whole schedule")
        compared += 1
    return compared


if __name__ == "__main__":
    trials = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    n_ops = int(sys.argv[3]) if len(sys.argv) > 3 else 60
    rep = {"trials": 0, "compared": 0, "failures": []}
    t0 = time.time()
    for trial in range(trials):
        ctx = Ctx()
        try:
            rep["compared"] += run_schedule(ctx, schedule(seed0 * 179424673 + trial, n_ops))
        except Exception as e:       # an AssertionError names the paths and the history
            rep["failures"].append(dict(trial=trial, seed=seed0 * 179424673 + trial, error=str(e)[:2000]))
        finally:
            try:
                ctx.close()
            except Exception:
                pass
        rep["trials"] += 1
        if len(rep["failures"]) > 5:
            break
    rep["wall_s"] = round(time.time() - t0, 1)
    print(json.dumps(rep))
