"""f5 measurement: the keyframe store's batched sub-map assembly (rgc_kf_assemble) on the MI355X against the same selection done with what the
library offered before it -- one rgc_transform_cloud(on_device) per (keyframe, kind) into a concatenated buffer, then rgc_voxelgrid(on_device)
-- at the loop-closure shape (101 history keyframes x corner + surf, 0.4 m leaf) and the surrounding-map shape (50 keyframes, corner map at
0.4 m and surf map at 0.8 m).  GPU time by HIP events on the context's stream, warm, median of --reps; the transform launch alone against the
measured HBM copy ceiling (6.29 TB/s); and, for information, the loop-closure ICP end to end from host clouds against device clouds.
    python scripts/bench_keyframes.py [--reps 30] [--n-az 900] [--out profiles/r07_keyframes.json]"""
import argparse, ctypes as C, json, math, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from rgc_slam_amd import _lib, keyframes

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--n-az", type=int, default=900)
ap.add_argument("--out", default=None)
args = ap.parse_args()
L = _lib.load()
hip = C.CDLL("libamdhip64.so")
vp, fp, dp, ip = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int)
hip.hipEventCreate.argtypes = [C.POINTER(vp)]; hip.hipEventRecord.argtypes = [vp, vp]; hip.hipEventSynchronize.argtypes = [vp]
hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), vp, vp]
COPY_CEILING = 6.29e12   # bytes/s, float4 copy measured on this part


def chk(rc, what=""):
    if rc != 0:
        raise RuntimeError("%s: status %d: %s" % (what, rc, L.rgc_last_error(h).decode()))


h = vp()
chk(L.rgc_create(0, None, C.byref(h)), "rgc_create")
stream = L.rgc_stream(h)
ev = [vp(), vp()]
for e in ev:
    assert hip.hipEventCreate(C.byref(e)) == 0


def gpu_ms(fn):
    """GPU time of what fn enqueues on the context's stream (and the host gaps between its launches), by HIP events"""
    chk(L.rgc_synchronize(h))
    assert hip.hipEventRecord(ev[0], stream) == 0
    fn()
    assert hip.hipEventRecord(ev[1], stream) == 0 and hip.hipEventSynchronize(ev[1]) == 0
    ms = C.c_float(0)
    assert hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]) == 0
    return float(ms.value)


def median_ms(fn, reps):
    for _ in range(3):
        fn()
    return float(np.median([gpu_ms(fn) for _ in range(reps)]))


def library_quaternion(pose):   # the chain of rgc_kf_push: float32 angles -> fp64 * rad2deg -> rgc_ypr2R -> Eigen's matrix-to-quaternion
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


def dalloc(nbytes):
    d = vp()
    chk(L.rgc_device_alloc(h, max(nbytes, 16), C.byref(d)), "rgc_device_alloc")
    return d


t0 = time.perf_counter()
ids, poses, clouds = keyframes.synthetic_keyframes(102, seed=20241008, n_az=args.n_az)
t_gen = time.perf_counter() - t0
store = keyframes.KeyframeStore(type("Owner", (), {"_h": h})())
for i in ids:
    store.push(i, poses[i], *clouds[i])
# the same body-frame clouds as separate device arrays, for the per-keyframe loop
d_body, quat = {}, {}
for i in ids:
    quat[i] = library_quaternion(poses[i])
    for k in range(2):
        a = clouds[i][k]
        d_body[(i, k)] = dalloc(a.nbytes)
        if len(a):
            chk(L.rgc_upload(h, d_body[(i, k)], a.ctypes.data, a.nbytes))
chk(L.rgc_synchronize(h))


def shape(name, sel, kinds, leaf):
    mask = sum(1 << k for k in kinds)
    sel_i = np.ascontiguousarray(sel, np.int32)
    n_raw = sum(len(clouds[i][k]) for i in sel for k in kinds)
    d_cat, d_out_a, d_out_b = dalloc(n_raw * 16), dalloc(n_raw * 16), dalloc(n_raw * 16)
    nr, no, no_b = C.c_int(0), C.c_int(0), C.c_int(0)

    def batched():
        chk(L.rgc_kf_assemble(h, sel_i.ctypes.data_as(ip), len(sel_i), mask, leaf, d_out_a, n_raw, 1, C.byref(nr), C.byref(no)), "rgc_kf_assemble")

    def transform_only():
        chk(L.rgc_kf_assemble(h, sel_i.ctypes.data_as(ip), len(sel_i), mask, 0.0, d_cat, n_raw, 1, C.byref(nr), C.byref(no_b)), "rgc_kf_assemble")

    def loop_transforms():
        off = 0
        for i in sel:
            t = poses[i][:3].astype(np.float64)
            for k in kinds:
                n = len(clouds[i][k])
                if n:
                    chk(L.rgc_transform_cloud(h, d_body[(i, k)], n, 16, quat[i].ctypes.data_as(dp), t.ctypes.data_as(dp), vp(d_cat.value + off * 16), 1), "rgc_transform_cloud")
                    off += n

    def loop():
        loop_transforms()
        chk(L.rgc_voxelgrid(h, d_cat, n_raw, 16, leaf, d_out_b, C.byref(no_b), 1), "rgc_voxelgrid")

    r = dict(shape=name, keyframes=len(sel), kinds=list(kinds), leaf=leaf, n_raw=n_raw, segments=sum(1 for i in sel for k in kinds if len(clouds[i][k])))
    r["loop_ms"] = median_ms(loop, args.reps)
    loop(); chk(L.rgc_synchronize(h))
    ref = np.empty((no_b.value, 4), np.float32); chk(L.rgc_download(h, ref.ctypes.data, d_out_b, ref.nbytes))
    r["batched_ms"] = median_ms(batched, args.reps)
    batched(); chk(L.rgc_synchronize(h))
    got = np.empty((no.value, 4), np.float32); chk(L.rgc_download(h, got.ctypes.data, d_out_a, got.nbytes))
    r["n_out"] = int(no.value)
    r["same_output_bit_for_bit"] = bool(got.shape == ref.shape and np.array_equal(got.view(np.uint32), ref.view(np.uint32)))
    r["loop_transforms_only_ms"] = median_ms(loop_transforms, args.reps)
    r["batched_transform_only_ms"] = median_ms(transform_only, args.reps)
    r["transform_bytes"] = 32 * n_raw
    r["transform_bytes_per_s"] = 32 * n_raw / (1e-3 * r["batched_transform_only_ms"])
    r["fraction_of_copy_ceiling"] = r["transform_bytes_per_s"] / COPY_CEILING
    r["speedup"] = r["loop_ms"] / r["batched_ms"]
    for d in (d_cat, d_out_a, d_out_b):
        L.rgc_device_free(h, d)
    return r


res = dict(workload="f5 keyframe store: batched sub-map assembly vs one rgc_transform_cloud per (keyframe, kind) + rgc_voxelgrid, device clouds",
           n_az=args.n_az, reps=args.reps, generation_s=round(t_gen, 1), copy_ceiling_bytes_per_s=COPY_CEILING, shapes=[])
res["shapes"].append(shape("loop closure: 101 history keyframes, corner + surf", ids[:101], (0, 1), 0.4))
res["shapes"].append(shape("surrounding corner map: 50 keyframes", ids[40:90], (0,), 0.4))
res["shapes"].append(shape("surrounding surf map: 50 keyframes", ids[40:90], (1,), 0.8))
res["batched_not_slower_at_every_shape"] = all(s["batched_ms"] <= s["loop_ms"] for s in res["shapes"])

# for information: f4 end to end, host clouds (assemble on the device, download, rgc_icp_align) against device clouds (rgc_icp_align_device)
prm = _lib.IcpParams(); L.rgc_default_icp_params(C.byref(prm))
src_d, tgt_d = store.assemble([ids[101]], (0, 1), device=True), store.assemble(ids[:101], (0, 1), leaf=0.4, device=True)
T, ir = np.zeros(16, np.float32), _lib.IcpResult()


def f4_device():
    s, t = store.assemble([ids[101]], (0, 1), device=True), store.assemble(ids[:101], (0, 1), leaf=0.4, device=True)
    chk(L.rgc_icp_align_device(h, s.ptr, len(s), t.ptr, len(t), 16, C.byref(prm), T.ctypes.data_as(fp), C.byref(ir)), "rgc_icp_align_device")
    s.close(); t.close()


def f4_host():
    s, t = store.assemble([ids[101]], (0, 1)), store.assemble(ids[:101], (0, 1), leaf=0.4)
    chk(L.rgc_icp_align(h, s.ctypes.data_as(fp), len(s), t.ctypes.data_as(fp), len(t), 16, C.byref(prm), T.ctypes.data_as(fp), C.byref(ir)), "rgc_icp_align")


def wall_ms(fn, reps=10):
    for _ in range(2):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


res["f4_end_to_end"] = dict(source_points=len(src_d), target_points=len(tgt_d), host_clouds_wall_ms=wall_ms(f4_host), device_clouds_wall_ms=wall_ms(f4_device),
                            iterations=int(ir.iterations), note="wall time of assemble + ICP from Python, median of 10; for information")
src_d.close(); tgt_d.close()
L.rgc_destroy(h)
line = json.dumps(res)
print(line)
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
