"""Outlier-filter measurement: GPU time (HIP events on the context's stream around WHOLE calls, median / min / max of --reps after 3 warm-ups) of rgc_outlier_statistical at mean_k = 8 / 20 / 50 and rgc_outlier_radius (exact counts, and with the early exit) on the 30 k-point scan and the 1 M-point map of the synthetic generator, cloud and outputs in device memory; beside each the route a caller had before these entry points existed: rgc_search_set_cloud + rgc_search_knn(mean_k + 1) of the cloud on itself into device memory, the keys' download and the host reduction (numpy), resp. rgc_search_set_cloud + rgc_search_radius with max_nn = min_neighbors + 1 and the offsets' download.  --variants G=LIB[,G=LIB ...]: the same measurement in a child process per developer build of the library with another lane-group size (RGC_EXTRA_FLAGS=-DRGC_LAB_OUTLIER_GROUP=G RGC_LIB_OUT=LIB python rgc-slam_amd/build.py), alternated with the product over --rounds rounds.
    python scripts/bench_outlier.py --out profiles/r22_outlier.json [--reps 9] [--variants 2=exp_flags/g2.so,8=exp_flags/g8.so]
Needs the GPU; reads nothing but the synthetic generator's clouds."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MEAN_KS = (8, 20, 50)
STD_MUL = 1.0
RADIUS, MIN_NB = 0.5, 5
SIZES = (("30 k-point scan", 30000, True), ("1 M-point map", 1000000, False))
PRODUCT_GROUP = 4   # rgck::FL_GROUP of csrc/rgc_filters.hip


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


def measure(reps, with_baseline):
    torch.cuda.set_device(0)
    import rgc_slam_amd.synth as synth
    from rgc_slam_amd import _lib, filters, search
    rows = []
    for name, n, is_scan in SIZES:
        world, tgt = synth.make_world_and_map(max(n, 30000))
        pts = synth.make_scan_n(world, np.eye(4), n)["xyz"] if is_scan else tgt
        pts = np.ascontiguousarray(pts[:n, :3], np.float32)
        n = len(pts)
        f = filters.StatisticalOutlierRemoval(0)
        L, h = f._L, f._h
        stream = L.rgc_stream(h)
        d_p = torch.from_numpy(pts).cuda()
        d_out, d_idx = torch.empty((n, 4), dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
        d_cnt = torch.empty(n, dtype=torch.int32, device="cuda")
        kept = C.c_int(0)
        info = _lib.OutlierInfo()
        row = dict(name=name, n=n, reps=reps, sor=[], ror=[])
        for mean_k in MEAN_KS:
            call = lambda: L.rgc_outlier_statistical(h, d_p.data_ptr(), n, 12, 1, mean_k, STD_MUL, 0, d_out.data_ptr(), d_idx.data_ptr(), None, C.byref(kept))
            assert call() == 0
            us = timed(stream, call, reps)
            L.rgc_outlier_get_info(h, C.byref(info))
            row["sor"].append(dict(mean_k=mean_k, us=us, kept=kept.value, candidates_per_point=info.candidates / n, grown=info.grown, cell=info.cell,
                                   checksum=int(d_idx[:kept.value].to(torch.int64).sum().item())))
        for exact in (1, 0):
            call = lambda: L.rgc_outlier_radius(h, d_p.data_ptr(), n, 12, 1, RADIUS, MIN_NB, 0, d_out.data_ptr(), d_idx.data_ptr(), d_cnt.data_ptr() if exact else None, C.byref(kept))
            assert call() == 0
            us = timed(stream, call, reps)
            L.rgc_outlier_get_info(h, C.byref(info))
            row["ror"].append(dict(radius=RADIUS, min_neighbors=MIN_NB, exact_counts=exact, us=us, kept=kept.value, candidates_per_point=info.candidates / n,
                                   checksum=int(d_idx[:kept.value].to(torch.int64).sum().item())))
        if with_baseline:
            t = search.KdTree(owner=f)
            base = dict(sor=[], ror=[])
            for mean_k in (k for k in MEAN_KS if k + 1 <= _lib.SEARCH_MAX_K):
                k1 = mean_k + 1
                r_idx, r_sq = torch.empty((n, k1), dtype=torch.int32, device="cuda"), torch.empty((n, k1), dtype=torch.float32, device="cuda")
                h_sq = np.empty((n, k1), np.float32)
                res = {}

                def device_part():
                    assert L.rgc_search_set_cloud(h, d_p.data_ptr(), n, 12, 1, 0.0) == 0
                    assert L.rgc_search_knn(h, d_p.data_ptr(), n, 12, 1, k1, r_idx.data_ptr(), r_sq.data_ptr()) == 0

                def whole():
                    device_part()
                    assert L.rgc_download(h, h_sq.ctypes.data, r_sq.data_ptr(), h_sq.nbytes) == 0
                    d = (np.sqrt(h_sq[:, 1:]).astype(np.float64).sum(axis=1) / mean_k).astype(np.float32).astype(np.float64)
                    mean = d.sum() / n
                    std = np.sqrt(max((np.dot(d, d) - d.sum() ** 2 / n) / (n - 1), 0.0))
                    res["mask"] = d <= mean + STD_MUL * std

                us_dev, us_all = timed(stream, device_part, reps), timed(stream, whole, reps)
                base["sor"].append(dict(mean_k=mean_k, us_search_only=us_dev, us=us_all, row_bytes=int(n) * k1 * 8, kept=int(res["mask"].sum())))
            total = C.c_longlong(0)
            d_off = torch.empty(n + 1, dtype=torch.int32, device="cuda")
            r_idx = torch.empty(n * (MIN_NB + 1), dtype=torch.int32, device="cuda")
            h_off = np.empty(n + 1, np.int32)
            res = {}

            def whole_ror():
                assert L.rgc_search_set_cloud(h, d_p.data_ptr(), n, 12, 1, 0.0) == 0
                assert L.rgc_search_radius(h, d_p.data_ptr(), n, 12, 1, RADIUS, MIN_NB + 1, 0, d_off.data_ptr(), r_idx.data_ptr(), None, n * (MIN_NB + 1), C.byref(total)) == 0
                assert L.rgc_download(h, h_off.ctypes.data, d_off.data_ptr(), h_off.nbytes) == 0
                res["mask"] = np.diff(h_off) - 1 >= MIN_NB

            base["ror"].append(dict(radius=RADIUS, min_neighbors=MIN_NB, us=timed(stream, whole_ror, reps), kept=int(res["mask"].sum())))
            row["baseline"] = base
            for b, x in zip(base["sor"], row["sor"]):      # (numpy's pairwise sums may move a threshold by an ulp: the kept counts agree to a handful)
                assert abs(b["kept"] - x["kept"]) <= 8, (b, x)
            assert base["ror"][0]["kept"] == row["ror"][0]["kept"] == row["ror"][1]["kept"]
        f.close()
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--variants", default="")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        print("ROWS " + json.dumps(measure(a.reps, with_baseline=not os.environ.get("RGC_HIP_LIB"))))
        return
    variants = [(PRODUCT_GROUP, None)] + [(int(v.split("=")[0]), os.path.abspath(v.split("=", 1)[1])) for v in a.variants.split(",") if v]
    runs = []
    for rnd in range(a.rounds):          # the builds alternate: other people's work shares the host
        for group, lib in variants:
            env = dict(os.environ)
            env.pop("RGC_HIP_LIB", None)
            if lib:
                env["RGC_HIP_LIB"] = lib
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps)], env=env, capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                sys.exit("the measurement of group %d failed (%d):\n%s" % (group, p.returncode, p.stderr[-2000:]))
            rows = json.loads([l for l in p.stdout.splitlines() if l.startswith("ROWS ")][-1][5:])
            runs.append(dict(lanes_per_point=group, library="product" if not lib else os.path.basename(lib), round=rnd, rows=rows))
    # every build must have computed the same thing: the kept sets are unique, so the counts and the index sums agree
    for run in runs[1:]:
        for r0, r1 in zip(runs[0]["rows"], run["rows"]):
            assert [(x["kept"], x["checksum"]) for x in r0["sor"] + r0["ror"]] == [(x["kept"], x["checksum"]) for x in r1["sor"] + r1["ror"]]
    res = dict(device=torch.cuda.get_device_name(0), method="HIP events on rgc_stream(ctx) around each WHOLE call, [median, min, max] microseconds of --reps repetitions after 3 "
               "warm-up calls; a filter call is its grid build (with the box's read-back), its chain of launches and the read-back of the number kept (synchronised); cloud and "
               "outputs in device memory; the baseline is the route through the search index with its downloads and the numpy reduction on the host inside the timed span "
               "(us_search_only: the index build and the search alone); one child process per library build, the builds alternated over the rounds", runs=runs)
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
