"""Search-index measurement: GPU time (HIP events on the context's stream, median / min / max of --reps after warm-up) of one rgc_search_knn at k = 1 / 5 / 20 / 32 and one rgc_search_radius at r = 0.5 / 1.0 -- capped at 32 and uncapped, sorted and unsorted -- for 30 k queries (a scan, in device memory, results into device memory) against 30 k and 1 M indexed points, with the candidates per query beside them, and next to each the library's own welded kernel on the same clouds where one exists: rgc_gicp_linearize's search for k = 1, rgc_mapreg_associate for k = 5 (host features: its copies are inside its time), rgc_gicpmp_linearize's gather for the radius.  --variants G=LIB[,G=LIB ...]: the same measurement in a child process per developer build of the library with another lane-group size (RGC_EXTRA_FLAGS=-DRGC_LAB_SEARCH_GROUP=G RGC_LIB_OUT=LIB python rgc-slam_amd/build.py), alternated with the product over --rounds rounds.
    python scripts/bench_search.py --out profiles/r21_search.json [--reps 9] [--variants 2=/tmp/g2.so,8=/tmp/g8.so,16=/tmp/g16.so]
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

KS = (1, 5, 20, 32)
RADII = (0.5, 1.0)
SIZES = (("30 k queries, 30 k indexed points", 30000, 30000), ("30 k queries, 1 M indexed points", 1000000, 30000))
PRODUCT_GROUP = 4   # rgck::SR_GROUP of csrc/rgc_search.hip


def timed(stream, fn, reps, warm=3):
    """[median, min, max] GPU microseconds between two events recorded on `stream` around fn()"""
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


def measure(reps, with_welded):
    torch.cuda.set_device(0)
    import rgc_slam_amd.synth as synth
    from rgc_slam_amd import search
    rows = []
    for name, nt, nq in SIZES:
        world, tgt = synth.make_world_and_map(nt)
        qry = np.ascontiguousarray(synth.make_scan_n(world, np.eye(4), nq)["xyz"][:, :3], np.float32)
        tgt = np.ascontiguousarray(tgt[:, :3], np.float32)
        t = search.KdTree(0)
        L, h = t._L, t._h
        stream = L.rgc_stream(h)
        t.setInputCloud(tgt)
        info = t.info()
        d_q = torch.from_numpy(qry).cuda()
        row = dict(name=name, n_indexed=len(tgt), n_queries=len(qry), reps=reps, cell=info["cell"], cells=info["cells"], knn=[], radius=[])
        d_idx, d_sq = torch.empty((nq, 32), dtype=torch.int32, device="cuda"), torch.empty((nq, 32), dtype=torch.float32, device="cuda")
        for k in KS:
            call = lambda: L.rgc_search_knn(h, d_q.data_ptr(), nq, 12, 1, k, d_idx.data_ptr(), d_sq.data_ptr())
            assert call() == 0
            us = timed(stream, call, reps)
            i = t.info()
            row["knn"].append(dict(k=k, us=us, candidates_per_query=i["candidates"] / nq, grown=i["grown"], checksum=int(d_idx[:, :k].to(torch.int64).sum().item())))
        d_off = torch.empty(nq + 1, dtype=torch.int32, device="cuda")
        for r in RADII:
            for max_nn in (32, 0):
                total = C.c_longlong(0)
                L.rgc_search_radius(h, d_q.data_ptr(), nq, 12, 1, r, max_nn, 1, None, None, None, 0, C.byref(total))
                n = total.value
                r_idx, r_sq = torch.empty(max(n, 1), dtype=torch.int32, device="cuda"), torch.empty(max(n, 1), dtype=torch.float32, device="cuda")
                for srt in (1, 0):
                    call = lambda: L.rgc_search_radius(h, d_q.data_ptr(), nq, 12, 1, r, max_nn, srt, d_off.data_ptr(), r_idx.data_ptr(), r_sq.data_ptr(), n, C.byref(total))
                    assert call() == 0
                    us = timed(stream, call, reps)
                    i = t.info()
                    row["radius"].append(dict(radius=r, max_nn=max_nn, sorted=srt, us=us, members_per_query=n / nq, candidates_per_query=i["candidates"] / nq,
                                              rows_sorted_long=i["rows_sorted_long"], checksum=int(r_idx[:n].to(torch.int64).sum().item())))
        t.close()
        if with_welded:
            from rgc_slam_amd.gicp import FastGICP, FastGICPMultiPoints
            from rgc_slam_amd.mapping import MapFeatureRegistration
            g = FastGICPMultiPoints(0)
            g.setInputTarget(tgt)
            g.setInputSource(qry)
            g.synchronize()
            gs = g._L.rgc_stream(g._h)
            T = np.eye(4)
            welded = dict(gicp_linearize_us_k1=timed(gs, lambda: FastGICP.linearize(g, T), reps))
            for r in RADII:
                g.setNeighborSearchRadius(r)
                welded["gicpmp_linearize_us_r%g" % r] = timed(gs, lambda: g.linearize(T), reps)
            g.close()
            m = MapFeatureRegistration(0)
            m.setInputMaps(tgt, tgt)
            feat = np.concatenate([qry, np.ones((nq, 1), np.float32)], axis=1)
            welded["mapreg_associate_us_k5"] = timed(m._L.rgc_stream(m._h), lambda: m.associate(feat, [0, 0, 0, 1], [0, 0, 0], "plane"), reps)
            m.close()
            row["welded"] = welded
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
        print("ROWS " + json.dumps(measure(a.reps, with_welded=not os.environ.get("RGC_HIP_LIB"))))
        return
    variants = [(PRODUCT_GROUP, None)] + [(int(v.split("=")[0]), v.split("=", 1)[1]) for v in a.variants.split(",") if v]
    runs = []
    for rnd in range(a.rounds if len(variants) > 1 else 1):          # the builds alternate: other people's work shares the host
        for group, lib in variants:
            env = dict(os.environ)
            env.pop("RGC_HIP_LIB", None)
            if lib:
                env["RGC_HIP_LIB"] = lib
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps)], env=env, capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                sys.exit("the measurement of group %d failed (%d):\n%s" % (group, p.returncode, p.stderr[-2000:]))
            rows = json.loads([l for l in p.stdout.splitlines() if l.startswith("ROWS ")][-1][5:])
            runs.append(dict(lanes_per_query=group, library="product" if not lib else os.path.basename(lib), round=rnd, rows=rows))
    # every build must have computed the same thing: the rows are unique under the order, so the index sums agree
    for run in runs[1:]:
        for r0, r1 in zip(runs[0]["rows"], run["rows"]):
            assert [x["checksum"] for x in r0["knn"]] == [x["checksum"] for x in r1["knn"]]
            assert [x["checksum"] for x in r0["radius"]] == [x["checksum"] for x in r1["radius"]]
    res = dict(device=torch.cuda.get_device_name(0), method="HIP events on rgc_stream(ctx) around each call, [median, min, max] microseconds of --reps repetitions after 3 warm-up "
               "calls; a call is the launches of one search, its read-out words' read-back and the copy of the rows into the caller's device buffers (synchronised); queries and "
               "results in device memory; one child process per library build, the builds alternated over the rounds", runs=runs)
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
