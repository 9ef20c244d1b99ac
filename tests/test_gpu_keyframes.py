"""The device keyframe store (f5: rgc_kf_*, rgc_icp_align_device, rgc_mapreg_set_maps_device) on the GPU.

Every comparison is over ALL points of a case, and every case's inputs are drawn from a seed named in the assertion message.
 1 transform: the unfiltered assembly against tests/kf_reference.py (count and order exact, fourth float bit-equal, x / y / z within
   pre_reference.ulp_bound: one fp32 ulp at the long-double value + 8 * 2^-53 (|p| + |t|), the bound tests/test_gpu_pre_routes.py uses for
   re-framing) and bit-equal to one rgc_transform_cloud call per (keyframe, kind) with the same quaternion (the parent commit's kernel);
 2 filter: bit-equal to pre_reference.voxelgrid over the GPU's own unfiltered assembly;   3 mutable poses;   4 the two device consumers
   against the host-pointer routes, bit for bit;   5 the boundary of the interface."""
import ctypes as C
import math

import numpy as np
import pytest

import kf_reference as kr
import pre_reference as pr
from rgc_slam_amd import _lib

pytestmark = pytest.mark.gpu

L = _lib.load()
fp, dp, ip = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int)
SIZES = [0, 1, 63, 64, 65, 255, 256, 257]


class Ctx:
    def __init__(self):
        self.h = C.c_void_p()
        rc = L.rgc_create(0, None, C.byref(self.h))
        assert rc == 0, rc

    def close(self):
        if self.h:
            L.rgc_destroy(self.h)
            self.h = None

    def err(self):
        return L.rgc_last_error(self.h).decode()

    def push(self, i, pose, clouds, stride_pad=0):
        arrs = []
        for a in clouds:
            a = np.asarray(a, np.float32).reshape(-1, 4)
            if stride_pad:
                b = np.full((len(a), 4 + stride_pad), 7.5, np.float32)
                b[:, :4] = a
                a = b
            arrs.append(np.ascontiguousarray(a))
        p = _lib.KfPose(*[float(v) for v in np.asarray(pose, np.float32)])
        return L.rgc_kf_push(self.h, int(i), C.byref(p), *sum(([a.ctypes.data if len(a) else None, len(a)] for a in arrs), []), 16 + 4 * stride_pad, 0)

    def set_poses(self, ids, poses):
        i = np.ascontiguousarray(ids, np.int32)
        p = np.ascontiguousarray(poses, np.float32).reshape(-1, 6)
        return L.rgc_kf_set_poses(self.h, i.ctypes.data_as(ip), p.ctypes.data_as(C.POINTER(_lib.KfPose)), len(i))

    def info(self):
        i = _lib.KfInfo()
        assert L.rgc_kf_get_info(self.h, C.byref(i)) == 0
        return i.n_keyframes, list(i.n_points), i.revision

    def assemble(self, ids, mask, leaf=0.0, cap=None, device=False):
        """(rc, n_raw, n_out, (n_out, 4) float32 or None)"""
        i = np.ascontiguousarray(ids, np.int32)
        ipp = i.ctypes.data_as(ip) if len(i) else None
        nr, no = C.c_int(-1), C.c_int(-1)
        if cap is None:
            L.rgc_kf_assemble(self.h, ipp, len(i), mask, 0.0, None, 0, 0, C.byref(nr), C.byref(no))
            cap = max(nr.value, 0)
        if device:
            d = C.c_void_p()
            assert L.rgc_device_alloc(self.h, max(cap, 1) * 16, C.byref(d)) == 0
            rc = L.rgc_kf_assemble(self.h, ipp, len(i), mask, leaf, d, cap, 1, C.byref(nr), C.byref(no))
            out = None
            if rc == 0:
                out = np.empty((no.value, 4), np.float32)
                assert L.rgc_download(self.h, out.ctypes.data, d, max(out.nbytes, 0)) == 0 if no.value else True
            L.rgc_device_free(self.h, d)
            return rc, nr.value, no.value, out
        out = np.full((max(cap, 1), 4), np.nan, np.float32)
        rc = L.rgc_kf_assemble(self.h, ipp, len(i), mask, leaf, out.ctypes.data if cap else None, cap, 0, C.byref(nr), C.byref(no))
        return rc, nr.value, no.value, (out[:no.value] if rc == 0 else out)

    def transform_cloud(self, pts, q, t):
        a = np.ascontiguousarray(pts, np.float32)
        out = np.empty((len(a), 4), np.float32)
        q, t = np.ascontiguousarray(q, np.float64), np.ascontiguousarray(t, np.float64)
        assert L.rgc_transform_cloud(self.h, a.ctypes.data, len(a), 16, q.ctypes.data_as(dp), t.ctypes.data_as(dp), out.ctypes.data, 0) == 0, self.err()
        return out

    def voxelgrid(self, pts, leaf):
        a = np.ascontiguousarray(pts, np.float32)
        out = np.empty((max(len(a), 1), 4), np.float32)
        n = C.c_int(0)
        rc = L.rgc_voxelgrid(self.h, a.ctypes.data, len(a), 16, float(leaf), out.ctypes.data, C.byref(n), 0)
        return rc, out[:n.value]


@pytest.fixture()
def ctx():
    c = Ctx()
    yield c
    c.close()


def library_quaternion(pose):
    """the quaternion the library's chain makes of a key pose, from its exported pieces: float32 fields -> fp64 * rad2deg -> rgc_ypr2R (degrees) -> Eigen's
    matrix-to-quaternion branches in fp64 (IEEE double operations: the same bits in numpy as in C++)"""
    p = np.asarray(pose, np.float32)
    deg = np.array([p[5], p[4], p[3]], np.float64) * (np.float64(180.0) / np.float64(math.pi))
    R = np.zeros(9)
    L.rgc_ypr2R(deg.ctypes.data_as(dp), R.ctypes.data_as(dp))
    t = R[0] + R[4] + R[8]
    if t > 0:
        t = np.sqrt(t + 1.0)
        w = 0.5 * t
        t = 0.5 / t
        return np.array([(R[7] - R[5]) * t, (R[2] - R[6]) * t, (R[3] - R[1]) * t, w])
    i = 0
    if R[4] > R[0]:
        i = 1
    if R[8] > R[i * 4]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    t = np.sqrt(R[i * 4] - R[j * 4] - R[k * 4] + 1.0)
    v = np.zeros(3)
    v[i] = 0.5 * t
    t = 0.5 / t
    w = (R[k * 3 + j] - R[j * 3 + k]) * t
    v[j] = (R[j * 3 + i] + R[i * 3 + j]) * t
    v[k] = (R[k * 3 + i] + R[i * 3 + k]) * t
    return np.array([v[0], v[1], v[2], w])


def draw_pose(rng, reach=2000.0):
    """translations out to `reach` metres (log-uniform in magnitude, any direction), every angle over its full range"""
    d = rng.normal(size=3)
    t = d / np.linalg.norm(d) * reach * 10.0 ** rng.uniform(-4, 0)
    return np.array([*t, rng.uniform(-np.pi, np.pi), rng.uniform(-np.pi / 2, np.pi / 2), rng.uniform(-np.pi, np.pi)], np.float32)


def draw_cloud(rng, n):
    a = np.empty((n, 4), np.float32)
    a[:, :3] = rng.normal(0, 1, (n, 3)) * rng.choice([0.5, 8.0, 40.0])
    a[:, 3] = rng.uniform(0, 255, n)
    return a


def draw_store(rng, nkf, reach=2000.0):
    ids = [int(v) for v in rng.choice(10 * nkf + 10, nkf, replace=False) - 3]          # the caller's ids: any ints, not 0..n-1
    clouds, poses = {}, {}
    for i in ids:
        ns = [int(rng.choice(SIZES + [int(rng.integers(1000, 5000))], p=[0.12] * 8 + [0.04])) for _ in range(3)]
        clouds[i] = [draw_cloud(rng, n) for n in ns]
        poses[i] = draw_pose(rng, reach)
    # empty kinds at the start, in the middle and at the end of a selection in store order
    clouds[ids[0]][0] = draw_cloud(rng, 0)
    clouds[ids[len(ids) // 2]] = [draw_cloud(rng, 0) for _ in range(3)] if nkf > 2 else clouds[ids[len(ids) // 2]]
    clouds[ids[-1]][2] = draw_cloud(rng, 0)
    if nkf == 1:
        clouds[ids[0]][1] = draw_cloud(rng, 257)
    return ids, clouds, poses


def fill(c, ids, clouds, poses):
    for n, i in enumerate(ids):
        assert c.push(i, poses[i], clouds[i], stride_pad=(n % 3)) == 0, c.err()      # strides 16, 20, 24 bytes


def check_raw(got, ref, wit, what):
    """got: the GPU's unfiltered assembly; ref: kf_reference.Assembly; wit: the per-(keyframe, kind) rgc_transform_cloud outputs, concatenated"""
    assert got.shape == (ref.n, 4), (what, got.shape, ref.n)
    assert np.array_equal(got[:, 3].view(np.uint32), ref.c.view(np.uint32)), what + ": the fourth float is not carried bit for bit / order"
    if ref.n == 0:
        return 0.0
    bound = pr.ulp_bound(ref.xyz, ref.p_abs, ref.t_abs)
    err = np.abs(got[:, :3].astype(np.float64) - ref.xyz).astype(np.float64)
    w, k = pr.worst_in_ulps(got[:, :3], ref.xyz)
    assert (err <= bound).all(), "%s: %.3f ulp at point %d, got %s reference %s" % (what, w, k // 3, got[k // 3, :3], ref.xyz[k // 3].astype(np.float64))
    assert np.array_equal(got.view(np.uint32), wit.view(np.uint32)), what + ": not bit-equal to rgc_transform_cloud per keyframe"
    return w


def orders(rng, ids):
    asc = sorted(ids)
    rep = [ids[int(v)] for v in rng.integers(0, len(ids), len(ids) + 3)]
    return dict(ascending=asc, descending=asc[::-1], repeated=rep, shuffled=[ids[int(v)] for v in rng.permutation(len(ids))])


@pytest.mark.parametrize("nkf", [1, 2, 7, 101, 400])
def test_transform(ctx, nkf):
    seed = 9100 + nkf
    rng = np.random.default_rng(seed)
    ids, clouds, poses = draw_store(rng, nkf)
    fill(ctx, ids, clouds, poses)
    assert ctx.info()[:2] == (nkf, [sum(len(clouds[i][k]) for i in ids) for k in range(3)])
    wit = {(i, k): (ctx.transform_cloud(clouds[i][k], library_quaternion(poses[i]), poses[i][:3].astype(np.float64)) if len(clouds[i][k]) else np.zeros((0, 4), np.float32))
           for i in ids for k in range(3)}
    worst = 0.0
    for oname, sel in orders(rng, ids).items():
        for mask in range(1, 8):
            what = "seed %d, %d keyframes, %s order, kind_mask %d" % (seed, nkf, oname, mask)
            ref = kr.assemble(clouds, poses, sel, mask)
            w = np.concatenate([wit[(i, k)] for i in sel for k in kr.kinds_of(mask)] + [np.zeros((0, 4), np.float32)])
            rc, n_raw, n_out, got = ctx.assemble(sel, mask, device=(mask % 2 == 0))
            assert rc == 0 and n_raw == n_out == ref.n, (what, rc, n_raw, n_out, ref.n, ctx.err())
            worst = max(worst, check_raw(got, ref, w, what))
    print("%d keyframes: largest difference to the long-double reference %.3f ulp" % (nkf, worst))


@pytest.mark.parametrize("spread", ["neighbourhood", "2 km"])
def test_filter(ctx, spread):
    seed = 9200 + len(spread)
    rng = np.random.default_rng(seed)
    ids, clouds, poses = draw_store(rng, 101, reach=60.0 if spread == "neighbourhood" else 2000.0)
    fill(ctx, ids, clouds, poses)
    sels = orders(rng, ids)
    leaves = [0.2, 0.4, 0.8, float(np.float32(rng.uniform(0.1, 1.5)))]
    for n, leaf in enumerate(leaves):
        for mask, oname in ((1, "ascending"), (2, "shuffled"), (3, "repeated"), (4, "descending"), (7, "shuffled")):
            what = "seed %d, %s, leaf %r, kind_mask %d, %s order" % (seed, spread, leaf, mask, oname)
            sel = sels[oname]
            rc, n_raw, _, raw = ctx.assemble(sel, mask)
            assert rc == 0, (what, ctx.err())
            rc, nr2, n_out, got = ctx.assemble(sel, mask, leaf=leaf, device=bool((n + mask) % 2))
            if spread == "2 km":                 # the same refusals as rgc_voxelgrid on the same cloud (a leaf grid beyond max_cells)
                rc_v, _ = ctx.voxelgrid(raw, leaf)
                assert rc == rc_v, (what, rc, rc_v)
                if rc != 0:
                    continue
            assert rc == 0 and nr2 == n_raw == len(raw), (what, rc, nr2, n_raw, ctx.err())
            ref = kr.filtered(raw, leaf)
            assert n_out == len(ref.out) and got.shape == ref.out.shape, (what, n_out, ref.out.shape)
            assert np.array_equal(got.view(np.uint32), ref.out.view(np.uint32)), what + ": " + pr.explain_mismatch(ref, got)


def test_mutable_poses(ctx):
    seed = 9300
    rng = np.random.default_rng(seed)
    ids, clouds, poses = draw_store(rng, 40)
    fill(ctx, ids, clouds, poses)
    sel = orders(rng, ids)["shuffled"]
    rc, _, _, before = ctx.assemble(sel, 7)
    assert rc == 0
    rev0 = ctx.info()[2]
    moved = [ids[int(v)] for v in rng.choice(len(ids), 9, replace=False)]
    new = dict(poses)
    for i in moved:
        new[i] = draw_pose(rng)
    assert ctx.set_poses(moved, [new[i] for i in moved]) == 0, ctx.err()
    assert ctx.info()[2] > rev0
    rc, _, _, after = ctx.assemble(sel, 7)
    assert rc == 0
    ref = kr.assemble(clouds, new, sel, 7)
    wit = np.concatenate([ctx.transform_cloud(clouds[i][k], library_quaternion(new[i]), new[i][:3].astype(np.float64)) for i in sel for k in range(3) if len(clouds[i][k])])
    check_raw(after, ref, wit, "seed %d after set_poses" % seed)
    for i, k, first, n in ref.segments:          # only the corrected keyframes' points moved
        same = np.array_equal(before[first:first + n].view(np.uint32), after[first:first + n].view(np.uint32))
        assert same == (i not in moved), (seed, i, k, same)
    # all or nothing: an unknown id or a non-finite pose among them changes no pose
    rev1 = ctx.info()[2]
    bad = np.array(new[moved[0]]); bad[4] = np.nan
    assert ctx.set_poses([moved[1], moved[0]], [poses[moved[1]], bad]) == _lib.ERR_NONFINITE
    assert ctx.set_poses([moved[1], 10 ** 6], [poses[moved[1]], poses[moved[1]]]) == _lib.ERR_INVALID
    assert ctx.info()[2] == rev1 and np.array_equal(ctx.assemble(sel, 7)[3].view(np.uint32), after.view(np.uint32))


# ---- 4 the consumers ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def drive():
    from rgc_slam_amd import keyframes
    return keyframes.synthetic_keyframes(102, seed=9400)


def _device_assembly(c, ids, mask, leaf):
    i = np.ascontiguousarray(ids, np.int32)
    nr, no = C.c_int(0), C.c_int(0)
    L.rgc_kf_assemble(c.h, i.ctypes.data_as(ip), len(i), mask, 0.0, None, 0, 0, C.byref(nr), C.byref(no))
    d = C.c_void_p()
    assert L.rgc_device_alloc(c.h, max(nr.value, 1) * 16, C.byref(d)) == 0
    assert L.rgc_kf_assemble(c.h, i.ctypes.data_as(ip), len(i), mask, leaf, d, nr.value, 1, C.byref(nr), C.byref(no)) == 0, c.err()
    host = np.empty((no.value, 4), np.float32)
    assert L.rgc_download(c.h, host.ctypes.data, d, host.nbytes) == 0
    return d, no.value, host


def test_loop_closure_icp_on_device_clouds(ctx, drive):
    ids, poses, clouds = drive
    for i in ids:
        assert ctx.push(i, poses[i], clouds[i]) == 0, ctx.err()
    latest, history = [ids[-1]], ids[:101]
    d_src, n_src, h_src = _device_assembly(ctx, latest, 3, 0.0)            # latestKeyFrameCloud: corner then surf, unfiltered (:2186-2191)
    d_tgt, n_tgt, h_tgt = _device_assembly(ctx, history, 3, 0.4)           # nearHistoryKeyFrameCloud through its leaf filter (:2209-2216)
    assert n_src > 100 and n_tgt > 1000
    prm = _lib.IcpParams()
    L.rgc_default_icp_params(C.byref(prm))
    out = []
    for route in ("device", "host", "device"):
        T, res = np.zeros(16, np.float32), _lib.IcpResult()
        if route == "device":
            rc = L.rgc_icp_align_device(ctx.h, d_src, n_src, d_tgt, n_tgt, 16, C.byref(prm), T.ctypes.data_as(fp), C.byref(res))
        else:
            rc = L.rgc_icp_align(ctx.h, h_src.ctypes.data_as(fp), n_src, h_tgt.ctypes.data_as(fp), n_tgt, 16, C.byref(prm), T.ctypes.data_as(fp), C.byref(res))
        assert rc == 0, (route, ctx.err())
        out.append((T.tobytes(), res.iterations, res.state, res.converged, res.n_correspondences, np.float64(res.fitness).tobytes()))
    assert out[0] == out[1] == out[2], [(o[1:5], np.frombuffer(o[5])) for o in out]
    assert out[0][1] >= 1 and out[0][4] > 100
    # the same checks as the host variant
    T, res = np.zeros(16, np.float32), _lib.IcpResult()
    assert L.rgc_icp_align_device(ctx.h, d_src, 0, d_tgt, n_tgt, 16, C.byref(prm), T.ctypes.data_as(fp), C.byref(res)) == _lib.ERR_TOO_FEW_POINTS
    assert L.rgc_icp_align_device(ctx.h, d_src, n_src, d_tgt, n_tgt, 10, C.byref(prm), T.ctypes.data_as(fp), C.byref(res)) == _lib.ERR_INVALID
    assert L.rgc_icp_align_device(ctx.h, None, n_src, d_tgt, n_tgt, 16, C.byref(prm), T.ctypes.data_as(fp), C.byref(res)) == _lib.ERR_INVALID
    for d in (d_src, d_tgt):
        L.rgc_device_free(ctx.h, d)


def test_surrounding_maps_feature_registration_on_device_clouds(ctx, drive):
    import mapreg_data as md
    from rgc_slam_amd import keyframes
    ids, poses, clouds = drive
    near = ids[40:90]                                                          # ~50 surrounding keyframes
    for i in ids:
        assert ctx.push(i, poses[i], clouds[i]) == 0, ctx.err()
    d_c, n_c, h_c = _device_assembly(ctx, near, 1, 0.4)                        # laserCloudCornerFromMapDS (:1608-1610)
    d_s, n_s, h_s = _device_assembly(ctx, near, 2, 0.8)                        # laserCloudSurfFromMapDS (:1612-1614)
    assert n_c > 50 and n_s > 200
    cur, last = ids[91], ids[90]

    def T_of(p):
        T = np.eye(4)
        T[:3, :3] = kr.rotation(p).astype(np.float64)
        T[:3, 3] = p[:3]
        return T
    rng = np.random.default_rng(9401)
    x0 = md.poses14(md.perturb(T_of(poses[cur]), rng), md.perturb(T_of(poses[last]), rng))
    feats = [np.ascontiguousarray(clouds[cur][0]), np.ascontiguousarray(clouds[cur][1]), np.ascontiguousarray(clouds[last][0]), np.ascontiguousarray(clouds[last][1])]
    out = []
    for route in ("device", "host", "device"):
        if route == "device":
            rc = L.rgc_mapreg_set_maps_device(ctx.h, d_c, n_c, d_s, n_s, 16)
        else:
            rc = L.rgc_mapreg_set_maps(ctx.h, h_c.ctypes.data_as(fp), n_c, h_s.ctypes.data_as(fp), n_s, 16)
        assert rc == 0, (route, ctx.err())
        x = np.ascontiguousarray(x0, np.float64).copy()
        rep = (_lib.MapregReport * 2)()
        gate = C.c_int(-1)
        args = sum(([f.ctypes.data_as(fp), len(f)] for f in feats), [])
        assert L.rgc_mapreg_optimize(ctx.h, *args, None, None, None, x.ctypes.data_as(dp), rep, C.byref(gate)) == 0, ctx.err()
        out.append((x.tobytes(), gate.value, bytes(rep)))
    assert out[0] == out[1] == out[2]
    assert out[0][1] == 0 and out[0][0] != np.ascontiguousarray(x0, np.float64).tobytes()      # the gate was met and the solve moved the poses
    assert L.rgc_mapreg_set_maps_device(ctx.h, d_c, 3, d_s, n_s, 16) == _lib.ERR_TOO_FEW_POINTS
    assert L.rgc_mapreg_set_maps_device(ctx.h, d_c, n_c, None, n_s, 16) == _lib.ERR_INVALID
    assert L.rgc_mapreg_set_maps_device(ctx.h, d_c, n_c, d_s, n_s, 6) == _lib.ERR_INVALID
    for d in (d_c, d_s):
        L.rgc_device_free(ctx.h, d)
    # the Python mirrors: a device cloud where a numpy array went, the same result
    from rgc_slam_amd.loop_closure import IterativeClosestPoint
    icp = IterativeClosestPoint(0)
    store = keyframes.KeyframeStore(icp)
    for i in ids[:30]:
        store.push(i, poses[i], *clouds[i])
    src_d, tgt_d = store.assemble([ids[29]], (0, 1), device=True), store.assemble(ids[:25], (0, 1), leaf=0.4, device=True)
    src_h, tgt_h = store.assemble([ids[29]], (0, 1)), store.assemble(ids[:25], (0, 1), leaf=0.4)
    assert np.array_equal(src_d.numpy(), src_h) and np.array_equal(tgt_d.numpy(), tgt_h)
    icp.setInputSource(src_d); icp.setInputTarget(tgt_d)
    Td, fd = icp.align().copy(), icp.getFitnessScore()
    icp.setInputSource(src_h); icp.setInputTarget(tgt_h)
    Th, fh = icp.align().copy(), icp.getFitnessScore()
    assert np.array_equal(Td, Th) and fd == fh
    src_d.close(); tgt_d.close(); store.close(); icp.close()


# ---- 5 the boundary -------------------------------------------------------------------------------------------------------------------------
def test_boundary(ctx):
    seed = 9500
    rng = np.random.default_rng(seed)
    # an empty store
    assert ctx.info()[:2] == (0, [0, 0, 0])
    assert ctx.assemble([], 7)[:3] == (0, 0, 0) and ctx.assemble([], 7, leaf=0.4)[:3] == (0, 0, 0)
    assert ctx.assemble([5], 7)[0] == _lib.ERR_INVALID
    ids, clouds, poses = draw_store(rng, 12)
    fill(ctx, ids, clouds, poses)
    rc, n_raw, _, full = ctx.assemble(ids, 7)
    assert rc == 0 and n_raw > 600
    # n_ids = 0, bad masks, unknown and duplicate ids, a non-finite pose, a stride that is none
    assert ctx.assemble([], 3)[:3] == (0, 0, 0)
    for mask in (0, 8, 255):
        assert ctx.assemble(ids, mask, cap=n_raw)[0] == _lib.ERR_INVALID
    rc, _, _, out = ctx.assemble(ids + [10 ** 6], 7, cap=n_raw)
    assert rc == _lib.ERR_INVALID and np.isnan(out).all(), "an unknown id: nothing is written"
    rev = ctx.info()[2]
    assert ctx.push(ids[3], poses[ids[3]], clouds[ids[3]]) == _lib.ERR_INVALID
    bad = np.array(poses[ids[0]]); bad[0] = np.inf
    assert ctx.push(10 ** 6, bad, clouds[ids[3]]) == _lib.ERR_NONFINITE
    a = draw_cloud(rng, 10)
    p = _lib.KfPose()
    for stride in (12, 18, 8192):
        assert L.rgc_kf_push(ctx.h, 10 ** 6, C.byref(p), a.ctypes.data, 10, None, 0, None, 0, stride, 0) == _lib.ERR_INVALID
    assert L.rgc_kf_push(ctx.h, 10 ** 6, C.byref(p), None, 10, None, 0, None, 0, 16, 0) == _lib.ERR_INVALID
    assert L.rgc_kf_push(ctx.h, 10 ** 6, C.byref(p), a.ctypes.data, -1, None, 0, None, 0, 16, 0) == _lib.ERR_INVALID
    assert ctx.info() == (12, [sum(len(clouds[i][k]) for i in ids) for k in range(3)], rev), "a refused push leaves the store as it was"
    # cap too small: the counts are reported, nothing is written, and the sized call succeeds
    rc, nr, no, out = ctx.assemble(ids, 7, cap=n_raw - 1)
    assert (rc, nr, no) == (_lib.ERR_INVALID, n_raw, n_raw) and np.isnan(out).all()
    rc, nr, no, out = ctx.assemble(ids, 7, leaf=50.0, cap=1)           # a 50 m leaf over poses out to 2 km: more than one leaf
    assert rc == _lib.ERR_INVALID and nr == n_raw and 1 < no <= n_raw and np.isnan(out).all()
    rc, _, no2, got = ctx.assemble(ids, 7, leaf=50.0, cap=no)
    assert rc == 0 and no2 == no and np.array_equal(got, kr.filtered(full, 50.0).out)
    # 2^27 by count arithmetic only: one keyframe of 2^20 points selected 129 times is refused before anything is allocated
    big = np.zeros((1 << 20, 4), np.float32)
    assert ctx.push(777777, poses[ids[0]], [big, big[:0], big[:0]]) == 0
    nr, no = C.c_int(-1), C.c_int(-1)
    sel = (C.c_int * 129)(*([777777] * 129))
    assert L.rgc_kf_assemble(ctx.h, sel, 129, 1, 0.0, None, 0, 0, C.byref(nr), C.byref(no)) == _lib.ERR_INVALID and "2^27" in ctx.err()
    assert L.rgc_kf_assemble(ctx.h, sel, 128, 1, 0.0, None, 0, 0, C.byref(nr), C.byref(no)) == _lib.ERR_INVALID and nr.value == 1 << 27    # (fits: only the room is missing)
    # reset, then reuse with the same ids
    assert L.rgc_kf_reset(ctx.h) == 0 and ctx.info()[:2] == (0, [0, 0, 0]) and ctx.assemble(ids[:1], 7)[0] == _lib.ERR_INVALID
    fill(ctx, ids, clouds, poses)
    assert np.array_equal(ctx.assemble(ids, 7)[3].view(np.uint32), full.view(np.uint32))


def test_growth_keeps_earlier_keyframes_and_contexts_are_independent(ctx):
    seed = 9600
    rng = np.random.default_rng(seed)
    other = Ctx()
    pose0, first = draw_pose(rng), draw_cloud(rng, 300)
    assert ctx.push(0, pose0, [first, first[:7], first[:0]]) == 0
    assert other.push(0, draw_pose(rng), [first[:5], first[:0], first[:0]]) == 0
    ref0 = ctx.assemble([0], 3)[3].copy()
    n, i = 300, 1
    while n < (1 << 20):                                   # the first allocation is 1 MiB (65536 points): four doublings and more
        c = draw_cloud(rng, n)
        assert ctx.push(i, draw_pose(rng), [c, c[:3], c[:1]]) == 0, ctx.err()
        last = (i, c)
        n, i = n * 2, i + 1
    assert np.array_equal(ctx.assemble([0], 3)[3].view(np.uint32), ref0.view(np.uint32)), "seed %d: the first keyframe changed while the store grew" % seed
    got = ctx.assemble([last[0]], 1)[3]
    assert np.array_equal(got[:, 3].view(np.uint32), last[1][:, 3].view(np.uint32))
    assert other.info()[:2] == (1, [5, 0, 0]) and other.assemble([0], 7)[1] == 5 and other.assemble([1], 7)[0] == _lib.ERR_INVALID
    other.close()


def test_store_calls_between_align_begin_and_end_do_not_disturb_the_solve(ctx):
    """documented choice: every rgc_kf_* call RUNS with a solve in flight; the solve's results are bit for bit those without them"""
    import rgc_slam_amd.synth as synth
    seed = 9700
    rng = np.random.default_rng(seed)
    world, base = synth.make_world_and_map(20000, seed=3)
    tgt = np.ascontiguousarray(base, np.float32)
    src = np.ascontiguousarray(base[::3] + np.float32(0.02), np.float32)
    ids, clouds, poses = draw_store(rng, 20, reach=60.0)
    guess = np.eye(4, dtype=np.float32)

    def solve(between):
        assert L.rgc_set_target(ctx.h, tgt.ctypes.data, len(tgt), 12) == 0 and L.rgc_set_source(ctx.h, src.ctypes.data, len(src), 12) == 0
        assert L.rgc_align_begin(ctx.h, guess.ctypes.data_as(fp), 1) == 0, ctx.err()
        if between:
            assert L.rgc_kf_reset(ctx.h) == 0
            fill(ctx, ids, clouds, poses)
            assert ctx.set_poses(ids[:3], [poses[i] for i in ids[3:6]]) == 0
            assert ctx.info()[0] == 20
            for leaf, dev in ((0.0, False), (0.4, False), (0.0, True), (0.8, True)):
                assert ctx.assemble(ids, 7, leaf=leaf, device=dev)[0] == 0, ctx.err()
        T, H, fit = np.zeros(16, np.float32), np.zeros(36), C.c_double(0)
        it, conv, lmf = C.c_int(0), C.c_int(0), C.c_int(0)
        assert L.rgc_align_end(ctx.h, T.ctypes.data_as(fp), H.ctypes.data_as(dp), C.byref(fit), C.byref(it), C.byref(conv), C.byref(lmf)) == 0, ctx.err()
        return T.tobytes(), H.tobytes(), np.float64(fit.value).tobytes(), it.value, conv.value, lmf.value

    solve(False)                 # (a context's first clouds measure their grids, later ones re-use them: compare like with like)
    plain, busy, again = solve(False), solve(True), solve(False)
    names = ("final_T", "final_H", "fitness", "iterations", "converged", "lm_failed")
    assert plain == again, "seed %d: two undisturbed solves differ in %s" % (seed, [n for n, a, b in zip(names, plain, again) if a != b])
    assert plain == busy, "seed %d: the solve with rgc_kf_* calls in between differs in %s" % (seed, [n for n, a, b in zip(names, plain, busy) if a != b])
    assert plain[3] >= 1
