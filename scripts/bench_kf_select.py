"""Keyframe-selection measurement on the MI355X (standalone, not bench.py).  Two questions:
  1. what rgc_uniform_sampling costs against rgc_voxelgrid -- the same chain but for its last launch -- on a 30 k-point sweep at 0.2 m and a
     1 M-point map at 0.4 m (device clouds, wall time of the whole call, alternating, median of --reps);
  2. what rgc_kf_select_surrounding / rgc_kf_select_global / rgc_kf_detect_loop cost at 1 k / 10 k / 100 k key poses (wall time of the whole call, mirror
     warm; and once with the mirror stale), against the same selections on the host: tests/us_reference.py (numpy), and -- since that reference was
     written to be read, not to be fast -- a plain numpy brute-force radius gate alone, the part a host loop cannot avoid.
Every device result is compared with the reference before it is timed.  Record, do not assert.
    python scripts/bench_kf_select.py [--reps 30] [--out profiles/r17_kf_select.json]"""
import argparse, ctypes as C, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from rgc_slam_amd import _lib, keyframes
import pre_cases as pc
import us_reference as us

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--sizes", type=int, nargs="*", default=[1000, 10000, 100000])
ap.add_argument("--out", default=None)
args = ap.parse_args()
L = _lib.load()
F = np.float32
ip = C.POINTER(C.c_int)


def wall_ms(fn, reps):
    for _ in range(3):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=float(np.median(t)), min_ms=float(np.min(t)), p90_ms=float(np.percentile(t, 90)))


def alternating_ms(fa, fb, reps):
    """two calls timed in turn, so that both see the same machine"""
    for _ in range(3):
        fa(); fb()
    ta, tb = [], []
    for _ in range(reps):
        t0 = time.perf_counter(); fa(); t1 = time.perf_counter(); fb(); t2 = time.perf_counter()
        ta.append((t1 - t0) * 1e3); tb.append((t2 - t1) * 1e3)
    return float(np.median(ta)), float(np.median(tb))


result = dict(reps=args.reps, filters=[], selections=[])

# ---- 1. UniformSampling against the leaf filter ----
h = C.c_void_p()
assert L.rgc_create(0, None, C.byref(h)) == 0
for name, cloud, leaf in (("sweep_30k", pc.sweep(n_az=2100)[:30000], 0.2), ("map_1M", pc.box_cloud(1000000, [-200, -200, -4], [200, 200, 36], 12, ground=0.6), 0.4)):
    cloud = np.ascontiguousarray(cloud, F)
    n = len(cloud)
    d_in, d_out, d_idx = C.c_void_p(), C.c_void_p(), C.c_void_p()
    for d, nbytes in ((d_in, cloud.nbytes), (d_out, 16 * n), (d_idx, 4 * n)):
        assert L.rgc_device_alloc(h, nbytes, C.byref(d)) == 0
    assert L.rgc_upload(h, d_in, cloud.ctypes.data, cloud.nbytes) == 0
    no = C.c_int(0)
    vg = lambda: L.rgc_voxelgrid(h, d_in, n, 16, C.c_float(leaf), d_out, C.byref(no), 1)
    usi = lambda: L.rgc_uniform_sampling(h, d_in, n, 16, C.c_float(leaf), d_out, d_idx, C.byref(no), 1)
    usn = lambda: L.rgc_uniform_sampling(h, d_in, n, 16, C.c_float(leaf), d_out, None, C.byref(no), 1)
    assert usi() == 0
    ref = us.uniform_sampling(cloud, leaf)
    idx = np.empty(no.value, np.int32)
    assert L.rgc_download(h, idx.ctypes.data, d_idx, idx.nbytes) == 0 and np.array_equal(idx, ref.index), name
    t_vg, t_us = alternating_ms(vg, usi, args.reps)
    t_vg2, t_usn = alternating_ms(vg, usn, args.reps)
    row = dict(case=name, n=n, leaf=leaf, leaves=int(no.value), fullest_leaf=ref.leaf.fullest, voxelgrid_ms=t_vg, uniform_sampling_ms=t_us,
               voxelgrid_again_ms=t_vg2, uniform_sampling_no_index_ms=t_usn)
    print(json.dumps(row)); result["filters"].append(row)
    for d in (d_in, d_out, d_idx):
        L.rgc_device_free(h, d)
L.rgc_destroy(h)


# ---- 2. the three selections ----
def drive(n, seed=5):
    """a drive that crosses itself: a slow Lissajous figure at ~0.5 m per key pose, with a little noise; the last pose lies near an early stretch"""
    rng = np.random.default_rng(seed)
    s = np.arange(n) * 0.5
    R = max(20.0, n * 0.5 / 25.0)
    poses = np.zeros((n, 6), F)
    poses[:, 0] = R * np.sin(s / R) + rng.normal(0, 0.02, n)
    poses[:, 1] = R * np.sin(2 * s / R) / 2 + rng.normal(0, 0.02, n)
    poses[:, 2] = rng.normal(0, 0.02, n)
    poses[:, 5] = np.arctan2(np.gradient(poses[:, 1]), np.gradient(poses[:, 0]))
    return poses, np.arange(n, dtype=np.int32)


for n in args.sizes:
    poses, ids = drive(n)
    store = keyframes.KeyframeStore()
    pts = np.zeros((4, 4), F)
    t0 = time.perf_counter()
    for i, p in zip(ids, poses):
        store.push(int(i), p, pts)
    push_ms = (time.perf_counter() - t0) * 1e3
    xyz = np.ascontiguousarray(poses[:, :3])
    d = store.travel(ids)[0]
    nf = np.full(n, 4)
    centre = poses[-1, :3]
    # correctness first
    w, w_n, _ = us.select_surrounding(xyz, ids, centre, 15.0, 0.3)
    got, n_in = store.select_surrounding(centre, 15.0, 0.3, return_count=True)
    assert n_in == w_n and np.array_equal(got, w), n
    wg, _ = us.select_global(xyz, ids, 0.5)
    assert np.array_equal(store.select_global(0.5), wg), n
    wl = us.detect_loop(xyz, ids, d, nf)
    gl = store.detect_loop()
    assert (gl["found"], gl["closest_id"], gl["n_in_radius"], list(gl["history_ids"])) == (wl["found"], wl["closest_id"], wl["n_in_radius"], wl["history_ids"]), n
    # raw C calls for the timing (the Python wrapper's allocations are not the library's)
    out = np.empty(n, np.int32)
    a, b = C.c_int(0), C.c_int(0)
    c3 = np.ascontiguousarray(centre, F)
    fp = C.POINTER(C.c_float)
    prm, cand = _lib.KfLoopParams(), _lib.KfLoopCandidate()
    L.rgc_default_kf_loop_params(C.byref(prm))
    hh = store._h
    sur = lambda: L.rgc_kf_select_surrounding(hh, c3.ctypes.data_as(fp), 15.0, 0.3, out.ctypes.data_as(ip), n, C.byref(a), C.byref(b))
    glo = lambda: L.rgc_kf_select_global(hh, 0.5, out.ctypes.data_as(ip), n, C.byref(b))
    loo = lambda: L.rgc_kf_detect_loop(hh, C.byref(prm), C.byref(cand), out.ctypes.data_as(ip), n, C.byref(b))
    one = np.ascontiguousarray(ids[:1])

    def stale_then(fn):
        def run():
            store.set_poses(one, poses[:1])       # the revision moves: the next selection uploads the mirror again
            fn()
        return run

    def host_gate():
        dd = xyz - centre
        return np.flatnonzero((dd * dd).sum(axis=1) < F(225.0))

    row = dict(n_keyframes=n, push_all_ms=push_ms, n_in_radius=int(w_n), n_surrounding=len(w), n_global=len(wg), loop_found=bool(wl["found"]),
               loop_n_in_radius=wl["n_in_radius"],
               device=dict(surrounding=wall_ms(sur, args.reps), global_=wall_ms(glo, args.reps), loop=wall_ms(loo, args.reps),
                           surrounding_stale_mirror=wall_ms(stale_then(sur), args.reps), loop_stale_mirror=wall_ms(stale_then(loo), args.reps),
                           set_poses_alone=wall_ms(lambda: store.set_poses(one, poses[:1]), args.reps)),
               host_reference=dict(surrounding=wall_ms(lambda: us.select_surrounding(xyz, ids, centre, 15.0, 0.3), max(3, args.reps // 3)),
                                   global_=wall_ms(lambda: us.select_global(xyz, ids, 0.5), max(3, args.reps // 3)),
                                   loop=wall_ms(lambda: us.detect_loop(xyz, ids, d, nf), max(3, args.reps // 3))),
               host_brute_force_gate_only=wall_ms(host_gate, args.reps))
    print(json.dumps(row)); result["selections"].append(row)
    store.close()

if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)
