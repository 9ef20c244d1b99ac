"""Euclidean-clustering measurement: GPU time (HIP events on the context's stream around WHOLE calls, median / min / max of --reps after 3 warm-ups) of rgc_cluster_extract at tolerances 0.2 / 0.5 / 1.0 m on the 30 k-point scan and the 1 M-point map of the synthetic generator, cloud and all three outputs in device memory, with n_components, largest and the candidates per point of every shape; beside each the only route a caller had before this entry point existed: rgc_search_set_cloud + rgc_search_radius of the cloud on itself (uncapped, unsorted; the size call and the fill call), the CSR's download and scipy.sparse.csgraph.connected_components on the host -- where the CSR exceeds 2^31 - 1 entries or the memory the refusal is the result.  --variants G=LIB[,G=LIB ...]: the fused call in a child process per developer build of the library with another lane-group size of k_cl_link (RGC_EXTRA_FLAGS=-DRGC_LAB_CLUSTER_GROUP=G RGC_LIB_OUT=LIB python rgc-slam_amd/build.py), alternated with the product over --rounds rounds.  --kernels: per-kernel times of the fused call on the 1 M-point map at 0.5 m from one more child under rocprofv3 --kernel-trace --stats.
    python scripts/bench_cluster.py --out profiles/r23_cluster.json [--reps 9] [--variants 2=g2.so,8=g8.so] [--kernels]
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

TOLERANCES = (0.2, 0.5, 1.0)
SIZES = (("30 k-point scan", 30000, True), ("1 M-point map", 1000000, False))
PRODUCT_GROUP = 4   # rgck::CL_GROUP of csrc/rgc_cluster.hip
INT_MAX = 2 ** 31 - 1


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
    cache = os.environ.get("RGC_BENCH_CLUSTER_CLOUDS")     # (the parent process generates the clouds once for its children)
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


def measure(reps, with_baseline, kernels_only=False):
    torch.cuda.set_device(0)
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    from rgc_slam_amd import _lib, search, segmentation
    rows = []
    for name, pts in clouds():
        n = len(pts)
        if kernels_only and n < 100000:
            continue
        f = segmentation.EuclideanClusterExtraction(0)
        L, h = f._L, f._h
        stream = L.rgc_stream(h)
        d_p = torch.from_numpy(pts).cuda()
        d_lab, d_off, d_idx = (torch.empty(n + 1, dtype=torch.int32, device="cuda") for _ in range(3))
        m = C.c_int(0)
        info = _lib.ClusterInfo()
        row = dict(name=name, n=n, reps=reps, fused=[])
        for tol in TOLERANCES if not kernels_only else (0.5,):
            call = lambda: L.rgc_cluster_extract(h, d_p.data_ptr(), n, 12, 1, tol, 1, INT_MAX, d_lab.data_ptr(), d_off.data_ptr(), d_idx.data_ptr(), C.byref(m))
            assert call() == 0
            if kernels_only:
                for _ in range(4):
                    assert call() == 0
                continue
            us = timed(stream, call, reps)
            L.rgc_cluster_get_info(h, C.byref(info))
            row["fused"].append(dict(tolerance=tol, us=us, n_components=info.n_components, n_clusters=m.value, largest=info.largest, candidates_per_point=info.candidates / n,
                                     cell=info.cell, checksum=int(d_lab[:n].to(torch.int64).sum().item()) + 31 * int(d_idx[:n].to(torch.int64).sum().item())))
        if with_baseline and not kernels_only:
            t = search.KdTree(owner=f)
            base = []
            for tol, fused in zip(TOLERANCES, row["fused"]):
                total = C.c_longlong(0)
                o_off = torch.empty(n + 1, dtype=torch.int32, device="cuda")
                assert L.rgc_search_set_cloud(h, d_p.data_ptr(), n, 12, 1, 0.0) == 0
                rc = L.rgc_search_radius(h, d_p.data_ptr(), n, 12, 1, tol, 0, 0, o_off.data_ptr(), o_off.data_ptr(), None, 0, C.byref(total))
                entry = dict(tolerance=tol, csr_entries=int(total.value))
                if total.value > INT_MAX or total.value * 12 > 48e9:
                    entry["refused"] = "the CSR has %d entries: beyond 2^31 - 1 (32-bit offsets) or the memory" % total.value
                    base.append(entry)
                    continue
                assert rc != 0 and total.value > 0                  # (the size call: cap = 0 is refused with the total set)
                cap = int(total.value)
                o_idx = torch.empty(cap, dtype=torch.int32, device="cuda")
                h_off, h_idx = np.empty(n + 1, np.int32), np.empty(cap, np.int32)
                res = {}

                def device_part():
                    assert L.rgc_search_set_cloud(h, d_p.data_ptr(), n, 12, 1, 0.0) == 0
                    L.rgc_search_radius(h, d_p.data_ptr(), n, 12, 1, tol, 0, 0, o_off.data_ptr(), o_idx.data_ptr(), None, 0, C.byref(total))     # the size call
                    assert L.rgc_search_radius(h, d_p.data_ptr(), n, 12, 1, tol, 0, 0, o_off.data_ptr(), o_idx.data_ptr(), None, cap, C.byref(total)) == 0

                def whole():
                    device_part()
                    assert L.rgc_download(h, h_off.ctypes.data, o_off.data_ptr(), h_off.nbytes) == 0
                    assert L.rgc_download(h, h_idx.ctypes.data, o_idx.data_ptr(), h_idx.nbytes) == 0
                    t0 = time.perf_counter()
                    res["n"], _ = connected_components(csr_matrix((np.ones(cap, np.int8), h_idx, h_off), shape=(n, n)), directed=False)
                    res["host_us"] = 1e6 * (time.perf_counter() - t0)

                few = max(3, reps // 3)
                entry.update(us_search_only=timed(stream, device_part, few, warm=1), us=timed(stream, whole, few, warm=1), host_components_us=res["host_us"], csr_bytes=cap * 4 + (n + 1) * 4,
                             n_components=int(res["n"]), reps=few)
                assert entry["n_components"] == fused["n_components"], (entry, fused)
                base.append(entry)
                del o_idx
            row["baseline"] = base
        f.close()
        rows.append(row)
    return rows


def kernel_times():
    """average nanoseconds per launch of every kernel of five fused calls on the 1 M-point map at tolerance 0.5, from a child under rocprofv3 --kernel-trace --stats"""
    with tempfile.TemporaryDirectory() as d:
        p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "cl", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), "--child", "--kernels-child"],
                           capture_output=True, text=True, timeout=900)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if p.returncode != 0 or not files:
            return dict(error="rocprofv3 run failed (%d): %s" % (p.returncode, p.stderr[-500:]))
        out = []
        for r in csv.DictReader(open(files[0])):
            out.append(dict(kernel=r["Name"].split("(")[0], calls=int(r["Calls"]), total_ns=int(float(r["TotalDurationNs"])), average_ns=float(r["AverageNs"]), max_ns=int(float(r["MaxNs"]))))
        return dict(note="all launches of 5 fused calls on the 1 M-point map at tolerance 0.5 in one process", kernels=out)


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
        rows = measure(a.reps, with_baseline=not os.environ.get("RGC_HIP_LIB"), kernels_only=a.kernels_child)
        print("ROWS " + json.dumps(rows))
        return
    variants = [(PRODUCT_GROUP, None)] + [(int(v.split("=")[0]), os.path.abspath(v.split("=", 1)[1])) for v in a.variants.split(",") if v]
    runs = []
    tmp = tempfile.TemporaryDirectory()
    os.environ["RGC_BENCH_CLUSTER_CLOUDS"] = os.path.join(tmp.name, "clouds.npz")
    np.savez(os.environ["RGC_BENCH_CLUSTER_CLOUDS"], **dict(clouds()))
    for rnd in range(a.rounds):          # the builds alternate: other people's work shares the host
        for group, lib in variants:
            env = dict(os.environ)
            env.pop("RGC_HIP_LIB", None)
            if lib:
                env["RGC_HIP_LIB"] = lib
            elif rnd > 0:
                env["RGC_HIP_LIB"] = os.path.join(ROOT, "rgc-slam_amd", "librgc_hip.so")     # (the baseline is measured once, in the first round)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps)], env=env, capture_output=True, text=True, timeout=1100)
            if p.returncode != 0:
                sys.exit("the measurement of group %d failed (%d):\n%s" % (group, p.returncode, p.stderr[-2000:]))
            rows = json.loads([l for l in p.stdout.splitlines() if l.startswith("ROWS ")][-1][5:])
            runs.append(dict(lanes_per_point=group, library="product" if not lib else os.path.basename(lib), round=rnd, rows=rows))
            print("round %d, %d lanes per point: done" % (rnd, group), file=sys.stderr, flush=True)
    # every build must have computed the same thing: the outputs are unique
    for run in runs[1:]:
        for r0, r1 in zip(runs[0]["rows"], run["rows"]):
            assert [(x["n_clusters"], x["checksum"]) for x in r0["fused"]] == [(x["n_clusters"], x["checksum"]) for x in r1["fused"]]
    res = dict(device=torch.cuda.get_device_name(0), method="HIP events on rgc_stream(ctx) around each WHOLE call, [median, min, max] microseconds of --reps repetitions after 3 "
               "warm-up calls; a fused call is its grid build (with the box's read-back), its chain of launches, the mid-chain read-back of the counts and the final wait; cloud and "
               "outputs in device memory, min_size 1, max_size INT_MAX, all three outputs; the baseline is the route through the search index (index build, the size call and the fill "
               "call of rgc_search_radius, uncapped and unsorted) with the CSR's download and scipy's connected_components on the host inside the timed span (us_search_only: the "
               "index build and the two search calls alone; fewer repetitions, 1 warm-up); one child process per library build, the builds alternated over the rounds", runs=runs)
    if a.kernels:
        res["kernel_times"] = kernel_times()
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
