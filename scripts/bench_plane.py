"""Plane-segmentation measurement: GPU time (HIP events on the context's stream around WHOLE calls, median / min / max of --reps after 3 warm-ups) of rgc_plane_segment (threshold 0.2 m, probability 0.99, seed 1, the generated stream, cloud and both outputs in device memory) on the 30 k-point scan and the 1 M-point map of the synthetic generator, for max_iterations 50 and 1000 at the automatic batch; a sweep of batch sizes (1 .. 1024) at max_iterations 1000; a breakdown -- refinement = the call with optimize 1 minus the call with optimize 0, per-launch cost = the slope of the call's time over its launches in the batch sweep, and with --kernels the per-kernel times of five calls per cloud from a child under rocprofv3 --kernel-trace --stats; and, for scale only, the wall time of the numpy reference (tests/plane_reference.py) on the same inputs.  --variants P=LIB[,P=LIB ...]: the same calls in a child process per developer build of the library with P points per thread of k_pl_score at every cloud size (RGC_EXTRA_FLAGS=-DRGC_LAB_PLANE_PPT=P RGC_LIB_OUT=LIB python rgc-slam_amd/build.py), alternated with the product over --rounds rounds.
    python scripts/bench_plane.py --out profiles/r24_plane.json [--reps 9] [--variants 1=p1.so,2=p2.so,8=p8.so] [--kernels]
Needs the GPU; reads nothing but the synthetic generator's clouds."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (("30 k-point scan", 30000, True), ("1 M-point map", 1000000, False))
ITERATIONS = (50, 1000)
BATCHES = (1, 4, 16, 64, 256, 1024)
THRESHOLD, SEED = 0.2, 1


def timed(stream, fn, reps, warm=3):
    """[median, min, max] microseconds between two events recorded on `stream` around fn() (host work inside fn delays the second event: it counts)"""
    s = torch.cuda.ExternalStream(stream, device=torch.device("cuda", 0))
    out = []
    for i in range(warm + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        fn()
        b.record(s)
        b.synchronize()
        if i >= warm:
            out.append(1000.0 * a.elapsed_time(b))
    return [float(np.median(out)), float(np.min(out)), float(np.max(out))]


def clouds():
    cache = os.environ.get("RGC_BENCH_PLANE_CLOUDS")     # (the parent process generates the clouds once for its children)
    if cache and os.path.exists(cache):
        z = np.load(cache)
        for name, _, _ in SIZES:
            yield name, z[name]
        return
    import rgc_slam_amd.synth as synth
    for name, n, is_scan in SIZES:
        world, tgt = synth.make_world_and_map(max(n, 30000))
        pts = synth.make_scan_n(world, np.eye(4), n)["xyz"] if is_scan else tgt
        yield name, np.ascontiguousarray(pts[:n, :3], np.float32)


def measure(reps, with_reference, kernels_only=False):
    torch.cuda.set_device(0)
    from rgc_slam_amd import _lib, segmentation
    rows = []
    for name, pts in clouds():
        n = len(pts)
        f = segmentation.SACSegmentation(0)
        L, h = f._L, f._h
        stream = L.rgc_stream(h)
        d_p = torch.from_numpy(pts).cuda()
        d_out, d_idx = torch.empty((n, 4), dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
        m, coeff, info = C.c_int(0), (C.c_double * 4)(), _lib.PlaneInfo()
        prm = _lib.PlaneParams()
        L.rgc_default_plane_params(C.byref(prm))
        prm.distance_threshold, prm.seed = THRESHOLD, SEED
        call = lambda: L.rgc_plane_segment(h, d_p.data_ptr(), n, 12, 1, C.byref(prm), None, 0, 1, coeff, d_out.data_ptr(), d_idx.data_ptr(), None, C.byref(m))

        def one(iters, batch, optimize):
            prm.max_iterations, prm.optimize = iters, optimize
            assert L.rgc_plane_set_batch(h, batch) == 0 and call() == 0
            us = timed(stream, call, reps)
            L.rgc_plane_get_info(h, C.byref(info))
            return dict(max_iterations=iters, batch=info.batch, optimize=optimize, us=us, iterations=info.iterations, positions=info.positions, launches=info.launches,
                        n_inliers=info.n_inliers, best_position=info.best_position, k=info.k, written=m.value, coeff=list(coeff),
                        checksum=int(d_idx[:m.value].to(torch.int64).sum().item()))
        row = dict(name=name, n=n, reps=reps)
        if kernels_only:
            prm.max_iterations = 1000
            for _ in range(5):
                assert call() == 0
            f.close()
            continue
        row["calls"] = [one(it, 0, opt) for it in ITERATIONS for opt in (1, 0)]
        row["batch_sweep"] = [one(1000, b, 1) for b in BATCHES]
        if with_reference:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import plane_reference as pr
            ref = []
            for it in ITERATIONS:
                t0 = time.perf_counter()
                r = pr.run(pts, pr.params(THRESHOLD, max_iterations=it, seed=SEED), None)
                ref.append(dict(max_iterations=it, wall_us=1e6 * (time.perf_counter() - t0), positions=r["positions"], n_inliers=len(r["inliers"])))
                same = [c for c in row["calls"] if c["max_iterations"] == it and c["optimize"] == 1][0]
                assert (same["positions"], same["best_position"]) == (r["positions"], r["best_position"]), (same, r["positions"], r["best_position"])
            row["numpy_reference"] = ref
        f.close()
        rows.append(row)
    return rows


def kernel_times():
    """average nanoseconds per launch of every kernel of five calls per cloud (max_iterations 1000, automatic batch), from a child under rocprofv3 --kernel-trace --stats"""
    with tempfile.TemporaryDirectory() as d:
        p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "pl", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), "--child", "--kernels-child"],
                           capture_output=True, text=True, timeout=600)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if p.returncode != 0 or not files:
            return dict(error="rocprofv3 run failed (%d): %s" % (p.returncode, p.stderr[-500:]))
        out = []
        for r in csv.DictReader(open(files[0])):
            out.append(dict(kernel=r["Name"].split("(")[0], calls=int(r["Calls"]), total_ns=int(float(r["TotalDurationNs"])), average_ns=float(r["AverageNs"]), max_ns=int(float(r["MaxNs"]))))
        return dict(note="all launches of 5 calls on each of the two clouds (max_iterations 1000, automatic batch) in one process: the 30 k-point scan's and the 1 M-point map's launches "
                    "of a kernel are averaged together", kernels=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--variants", default="")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--kernels-child", action="store_true")
    a = ap.parse_args()
    if a.child:
        rows = measure(a.reps, with_reference=not os.environ.get("RGC_HIP_LIB"), kernels_only=a.kernels_child)
        print("ROWS " + json.dumps(rows))
        return
    variants = [("product", None)] + [(v.split("=")[0], os.path.abspath(v.split("=", 1)[1])) for v in a.variants.split(",") if v]
    runs = []
    tmp = tempfile.TemporaryDirectory()
    os.environ["RGC_BENCH_PLANE_CLOUDS"] = os.path.join(tmp.name, "clouds.npz")
    np.savez(os.environ["RGC_BENCH_PLANE_CLOUDS"], **dict(clouds()))
    for rnd in range(a.rounds):          # the builds alternate: other people's work shares the host
        for ppt, lib in variants:
            env = dict(os.environ)
            env.pop("RGC_HIP_LIB", None)
            if lib:
                env["RGC_HIP_LIB"] = lib
            elif rnd > 0:
                env["RGC_HIP_LIB"] = os.path.join(ROOT, "rgc-slam_amd", "librgc_hip.so")     # (the numpy reference is timed once, in the first round)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps)], env=env, capture_output=True, text=True, timeout=1100)
            if p.returncode != 0:
                sys.exit("the measurement of %s failed (%d):\n%s" % (ppt, p.returncode, p.stderr[-2000:]))
            rows = json.loads([l for l in p.stdout.splitlines() if l.startswith("ROWS ")][-1][5:])
            runs.append(dict(points_per_thread=ppt if lib else "product (1 below 65 536 points, 4 from there)", library="product" if not lib else os.path.basename(lib), round=rnd, rows=rows))
            print("round %d, %s: done" % (rnd, ppt), file=sys.stderr, flush=True)
    # every build and every batch size must have computed the same thing
    for run in runs:
        for r0, r1 in zip(runs[0]["rows"], run["rows"]):
            key = lambda x: (x["positions"], x["best_position"], x["written"], x["checksum"], x["coeff"])
            assert [key(x) for x in r0["calls"]] == [key(x) for x in r1["calls"]]
            assert len({json.dumps(key(x)) for x in r1["batch_sweep"]}) == 1
    res = dict(device=torch.cuda.get_device_name(0), method="HIP events on rgc_stream(ctx) around each WHOLE call, [median, min, max] microseconds of --reps repetitions after 3 warm-up "
               "calls; a call is its batches (k_pl_models, k_pl_score and one read-back each, the decision replayed on the host between them), the best model's upload, the refinement "
               "(optimize 1), the flags, their scan, the records and the final read-back; cloud and both outputs in device memory, negative = 1 (the ground-removed cloud), threshold 0.2 m, "
               "probability 0.99, seed 1, the generated stream; numpy_reference: wall time of tests/plane_reference.py on the same inputs on the host, for scale only; one child process "
               "per library build, the builds alternated over the rounds", runs=runs)
    if a.kernels:
        res["kernel_times"] = kernel_times()
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
