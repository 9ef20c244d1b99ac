"""Normal-estimation measurement: GPU time (HIP events on the context's stream around WHOLE calls, median / min / max of --reps after 3 warm-ups) of rgc_normal_estimate at k = 10 / 20 and radius 0.3 / 0.5 / 1.0 on the 30 k-point scan and the 1 M-point map of the synthetic generator, each cloud its own surface, cloud and normals in device memory; beside each the route a caller had before this entry point existed: rgc_search_set_cloud + rgc_search_knn(k) resp. rgc_search_radius (unsorted, sized by a first call) of the cloud on itself into device memory, the rows' download and the host reduction (numpy: the gathered neighbours' moments about the query in fp64, numpy.linalg.eigh, the flip towards the viewpoint), at --base-reps repetitions after one warm-up.  --variants G=LIB[,G=LIB ...]: the same measurement (without the baseline) in a child process per developer build of the library with another lane-group size on both routes (RGC_EXTRA_FLAGS="-DRGC_LAB_NORMAL_GROUP=G -DRGC_LAB_NORMAL_RADIUS_GROUP=G" RGC_LIB_OUT=LIB python rgc-slam_amd/build.py), alternated with the product over --rounds rounds; a variant whose number is the product's 4 is any other developer build (RGC_EXTRA_FLAGS=-DRGC_LAB_NORMAL_INPUT_ORDER: the self-surface cloud walked in input order, not in the grid's sorted order).
    python scripts/bench_normals.py --out profiles/r25_normals.json [--reps 9] [--variants 2=exp_flags/nrm_g2.so,8=exp_flags/nrm_g8.so,4=exp_flags/nrm_input_order.so]
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

KS = (10, 20)
RADII = (0.3, 0.5, 1.0)
SIZES = (("30 k-point scan", 30000, True), ("1 M-point map", 1000000, False))
PRODUCT_GROUP = 4   # rgck::NR_GROUP and NR_RGROUP of csrc/rgc_normals.hip


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


def host_normals(P, off, idx, block=65536):
    """the host reduction of downloaded rows (CSR): moments about the query in fp64 (a block of queries at a time: the gathered rows of a 1 M-point map do not
    fit memory at once), eigh, the flip towards the origin; NaN rows under three members"""
    n = len(P)
    m = np.diff(off)
    P64 = P.astype(np.float64)
    sums = np.zeros((n, 9))
    for q0 in range(0, n, block):
        q1 = min(q0 + block, n)
        a, b = int(off[q0]), int(off[q1])
        if b == a:
            continue
        d = P64[idx[a:b]] - np.repeat(P64[q0:q1], m[q0:q1], axis=0)
        terms = np.concatenate([d, d[:, [0, 0, 0, 1, 1, 2]] * d[:, [0, 1, 2, 1, 2, 2]]], axis=1)
        rows = np.flatnonzero(m[q0:q1] > 0)
        sums[q0 + rows] = np.add.reduceat(terms, off[q0 + rows] - a, axis=0)
    mm = np.maximum(m, 1)[:, None].astype(np.float64)
    mean = sums[:, :3] / mm
    c6 = sums[:, 3:] / mm - mean[:, [0, 0, 0, 1, 1, 2]] * mean[:, [0, 1, 2, 1, 2, 2]]
    S = np.empty((n, 3, 3))
    for j, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        S[:, a, b] = S[:, b, a] = c6[:, j]
    w, V = np.linalg.eigh(S)
    nrm = V[:, :, 0]
    nrm = np.where((((-P64) * nrm).sum(axis=1) < 0)[:, None], -nrm, nrm)
    out = np.concatenate([nrm, (np.abs(w[:, 0]) / np.maximum(np.trace(S, axis1=1, axis2=2), 1e-300))[:, None]], axis=1).astype(np.float32)
    out[m < 3] = np.nan
    return out


def measure(reps, base_reps, with_baseline):
    torch.cuda.set_device(0)
    import rgc_slam_amd.synth as synth
    from rgc_slam_amd import _lib, features, search
    rows = []
    for name, n, is_scan in SIZES:
        world, tgt = synth.make_world_and_map(max(n, 30000))
        pts = synth.make_scan_n(world, np.eye(4), n)["xyz"] if is_scan else tgt
        pts = np.ascontiguousarray(pts[:n, :3], np.float32)
        n = len(pts)
        f = features.NormalEstimation(0)
        L, h = f._L, f._h
        stream = L.rgc_stream(h)
        d_p = torch.from_numpy(pts).cuda()
        d_n4 = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        d_cnt = torch.empty(n, dtype=torch.int32, device="cuda")
        valid = C.c_int(0)
        info = _lib.NormalInfo()
        row = dict(name=name, n=n, reps=reps, runs=[])
        prm = _lib.NormalParams()
        for k, radius in [(k, 0.0) for k in KS] + [(0, r) for r in RADII]:
            L.rgc_default_normal_params(C.byref(prm))
            prm.k, prm.radius = k, radius
            call = lambda: L.rgc_normal_estimate(h, d_p.data_ptr(), n, 12, None, 0, 0, 1, C.byref(prm), d_n4.data_ptr(), None, None, d_cnt.data_ptr(), C.byref(valid))
            assert call() == 0
            us = timed(stream, call, reps)
            L.rgc_normal_get_info(h, C.byref(info))
            members = int(d_cnt.to(torch.int64).sum().item())
            got = d_n4.cpu().numpy()
            run = dict(k=k, radius=radius, us=us, n_valid=valid.value, members_per_query=members / n, candidates_per_query=info.candidates / n, grown=info.grown, cell=info.cell,
                       members=members)
            if with_baseline:
                t = search.KdTree(owner=f)
                res = {}
                if k:
                    r_idx, r_sq = torch.empty((n, k), dtype=torch.int32, device="cuda"), torch.empty((n, k), dtype=torch.float32, device="cuda")
                    h_idx = np.empty((n, k), np.int32)

                    def device_part():
                        assert L.rgc_search_set_cloud(h, d_p.data_ptr(), n, 12, 1, 0.0) == 0
                        assert L.rgc_search_knn(h, d_p.data_ptr(), n, 12, 1, k, r_idx.data_ptr(), r_sq.data_ptr()) == 0

                    def whole():
                        device_part()
                        assert L.rgc_download(h, h_idx.ctypes.data, r_idx.data_ptr(), h_idx.nbytes) == 0
                        res["n4"] = host_normals(pts, np.arange(n + 1, dtype=np.int64) * k, h_idx.reshape(-1))
                    row_bytes = int(n) * k * 4
                else:
                    total = C.c_longlong(0)
                    d_off = torch.empty(n + 1, dtype=torch.int32, device="cuda")
                    r_idx = torch.empty(max(members, 1), dtype=torch.int32, device="cuda")
                    h_off, h_idx = np.empty(n + 1, np.int32), np.empty(members, np.int32)

                    def device_part():
                        assert L.rgc_search_set_cloud(h, d_p.data_ptr(), n, 12, 1, 0.0) == 0
                        rc = L.rgc_search_radius(h, d_p.data_ptr(), n, 12, 1, radius, 0, 0, None, None, None, 0, C.byref(total))     # the size-then-fill protocol's first call
                        assert rc in (0, _lib.ERR_INVALID) and total.value == members
                        assert L.rgc_search_radius(h, d_p.data_ptr(), n, 12, 1, radius, 0, 0, d_off.data_ptr(), r_idx.data_ptr(), None, members, C.byref(total)) == 0

                    def whole():
                        device_part()
                        assert L.rgc_download(h, h_off.ctypes.data, d_off.data_ptr(), h_off.nbytes) == 0
                        if members:
                            assert L.rgc_download(h, h_idx.ctypes.data, r_idx.data_ptr(), h_idx.nbytes) == 0
                        res["n4"] = host_normals(pts, h_off.astype(np.int64), h_idx)
                    row_bytes = (int(n) + 1 + members) * 4
                us_dev, us_all = timed(stream, device_part, base_reps, warm=1), timed(stream, whole, base_reps, warm=1)
                # the two routes computed the same thing: the same rows are valid, and the normals agree wherever numpy's solver and the library's pick the same axis
                both = ~np.isnan(got[:, 0]) & ~np.isnan(res["n4"][:, 0])
                assert np.array_equal(np.isnan(got[:, 0]), np.isnan(res["n4"][:, 0]))
                agree = float((np.abs((got[both, :3] * res["n4"][both, :3]).sum(axis=1)) > 0.999).mean()) if both.any() else 1.0
                run["baseline"] = dict(us_search_only=us_dev, us=us_all, reps=base_reps, row_bytes=row_bytes, normals_within_2_6_degrees=agree)
                t.clear()
            run["checksum"] = int(np.nan_to_num(got[:, :3]).astype(np.float64).__abs__().sum() * 1e6)
            row["runs"].append(run)
        f.close()
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--base-reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--variants", default="")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--no-baseline", action="store_true")
    a = ap.parse_args()
    if a.child:
        print("ROWS " + json.dumps(measure(a.reps, a.base_reps, with_baseline=not a.no_baseline)))
        return
    variants = [(PRODUCT_GROUP, None)] + [(int(v.split("=")[0]), os.path.abspath(v.split("=", 1)[1])) for v in a.variants.split(",") if v]
    runs = []
    for rnd in range(a.rounds):          # the builds alternate: other people's work shares the host
        for group, lib in variants:
            env = dict(os.environ)
            env.pop("RGC_HIP_LIB", None)
            if lib:
                env["RGC_HIP_LIB"] = lib
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--base-reps", str(a.base_reps)]
            if lib or rnd > 0:           # the baseline once, with the product
                cmd.append("--no-baseline")
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1100)
            if p.returncode != 0:
                sys.exit("the measurement of group %d failed (%d):\n%s" % (group, p.returncode, p.stderr[-2000:]))
            rows = json.loads([l for l in p.stdout.splitlines() if l.startswith("ROWS ")][-1][5:])
            runs.append(dict(lanes_per_query=group, library="product" if not lib else os.path.basename(lib), round=rnd, rows=rows))
            print("round %d, %d lanes per query: done" % (rnd, group), file=sys.stderr, flush=True)
    # every build must have computed the same thing: the k route's bits do not depend on the group size, the radius route's counts do not
    for run in runs[1:]:
        for r0, r1 in zip(runs[0]["rows"], run["rows"]):
            assert [(x["n_valid"], x["members"]) for x in r0["runs"]] == [(x["n_valid"], x["members"]) for x in r1["runs"]]
            assert [x["checksum"] for x in r0["runs"] if x["k"]] == [x["checksum"] for x in r1["runs"] if x["k"]]
    res = dict(device=torch.cuda.get_device_name(0), method="HIP events on rgc_stream(ctx) around each WHOLE call, [median, min, max] microseconds of --reps repetitions after 3 "
               "warm-up calls; a call is its grid build (with the box's read-back), the fused launch and the read-back of the read-out words (synchronised); cloud, normals and "
               "counts in device memory; the baseline is the route through the search index with its downloads and the numpy reduction on the host inside the timed span, "
               "--base-reps repetitions after one warm-up (us_search_only: the index build and the search alone); one child process per library build, the builds alternated "
               "over the rounds", runs=runs)
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
