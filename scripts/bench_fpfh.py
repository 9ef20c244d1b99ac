"""FPFH measurement: GPU time (HIP events on the context's stream around WHOLE calls, median / min / max of --reps after 3 warm-ups) of rgc_fpfh_estimate on the 30 k-point scan of the synthetic generator as its own surface at three radii (about 10, 30 and 100 members per point) and of 500 keypoints against the 1 M-point map, clouds, normals (rgc_normal_estimate's out_normal4 where it was left, k = 10) and descriptors in device memory; beside each the route a caller had before this entry point existed: rgc_search_set_cloud + rgc_search_radius (sized by a first call) into device memory, the rows' and the normals' download and the two passes in numpy on the host (fp64, vectorised over the pairs), at --base-reps repetitions after one warm-up; and the scan's calls again at fixed cell sizes 0.5 / 1 / 2 m of the call's grid (rgc_fpfh_set_cell).  --kernels: the per-kernel times of five calls per workload, each workload in a child of its own under rocprofv3 --kernel-trace --stats.  --variants NAME=LIB[,NAME=LIB ...]: the same measurement (without the baseline) in a child process per developer build of the library (another lane-group size of the SPFH pass, RGC_EXTRA_FLAGS=-DRGC_LAB_FPFH_SPFH_GROUP=G, or of the combine pass, -DRGC_LAB_FPFH_COMBINE_GROUP=G, RGC_LIB_OUT=LIB python rgc-slam_amd/build.py), alternated with the product over --rounds rounds.
    python scripts/bench_fpfh.py --out profiles/r26_fpfh.json [--reps 9] [--kernels] [--variants spfh4=exp_flags/fpfh_s4.so,combine8=exp_flags/fpfh_c8.so]
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

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCAN_RADII = (0.16, 0.3, 0.65)
MAP_RADIUS = 1.0
N_KEYPOINTS = 500
CELLS = (0.5, 1.0, 2.0)
WORKLOADS = [("30 k-point scan, its own surface", "scan", r) for r in SCAN_RADII] + [("500 keypoints against the 1 M-point map", "map", MAP_RADIUS)]


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


def host_spfh(T, N, rows_of, off, idx, block=1 << 18):
    """the first pass on the host from downloaded rows (CSR over the surface points rows_of): (counts (len(rows_of), 33), m) in fp64, vectorised over the pairs"""
    m = np.diff(off)
    counts = np.zeros((len(rows_of), 33), np.int64)
    T64, N64 = T.astype(np.float64), N.astype(np.float64)
    ok_n = np.isfinite(N64).all(axis=1)
    row = np.repeat(np.arange(len(rows_of)), m)
    for a in range(0, len(idx), block):
        r, t = row[a:a + block], idx[a:a + block]
        s = rows_of[r]
        d = T64[t] - T64[s]
        f4 = np.sqrt((d * d).sum(axis=1))
        use = (f4 > 0) & ok_n[s] & ok_n[t]
        r, s, t, d, f4 = r[use], s[use], t[use], d[use], f4[use]
        A, B = N64[s], N64[t]
        c1, c2 = (A * d).sum(axis=1), (B * d).sum(axis=1)
        sw = np.abs(c1) < np.abs(c2)
        u, n2 = np.where(sw[:, None], B, A), np.where(sw[:, None], A, B)
        d = np.where(sw[:, None], -d, d)
        f3 = np.where(sw, -c2, c1) / f4
        v = np.cross(d, u)
        vn = np.sqrt((v * v).sum(axis=1))
        keep = vn > 0
        r, u, n2, v, f3 = r[keep], u[keep], n2[keep], v[keep] / vn[keep, None], f3[keep]
        w = np.cross(u, v)
        f2 = (v * n2).sum(axis=1)
        f1 = np.arctan2((w * n2).sum(axis=1), (u * n2).sum(axis=1))
        for blk, x in enumerate(((f1 + np.pi) / (2 * np.pi), (f2 + 1) * 0.5, (f3 + 1) * 0.5)):
            b = np.clip(np.floor(11 * x), 0, 10).astype(np.int64)
            counts += np.bincount(r * 33 + blk * 11 + b, minlength=counts.size).reshape(counts.shape)
    return counts, m


def host_fpfh(counts_at, m_at, off, idx, key):
    """the second pass on the host: counts_at / m_at indexed by surface point; (nq, 33) float32"""
    nq = len(off) - 1
    with np.errstate(divide="ignore"):
        A = counts_at * (100.0 / np.maximum(m_at - 1, 1))[:, None]
    use = np.flatnonzero((key > 0) & (m_at[idx] > 1))
    row = np.repeat(np.arange(nq), np.diff(off))[use]
    F = np.zeros((nq, 33))
    terms = A[idx[use]] / key[use].astype(np.float64)[:, None]
    for b in range(33):
        F[:, b] = np.bincount(row, terms[:, b], minlength=nq)
    out = np.zeros((nq, 33))
    for blk in range(3):
        s = F[:, blk * 11:blk * 11 + 11].sum(axis=1)
        nz = s != 0
        out[nz, blk * 11:blk * 11 + 11] = F[nz, blk * 11:blk * 11 + 11] * (100.0 / s[nz])[:, None]
    out[np.diff(off) == 0] = np.nan
    return out.astype(np.float32)


def clouds():
    import rgc_slam_amd.synth as synth
    world, tgt = synth.make_world_and_map(1000000)
    scan = np.ascontiguousarray(synth.make_scan_n(world, np.eye(4), 30000)["xyz"][:, :3], np.float32)
    tgt = np.ascontiguousarray(tgt[:, :3], np.float32)
    rng = np.random.default_rng(26)
    keys = (tgt[::len(tgt) // N_KEYPOINTS][:N_KEYPOINTS] + rng.normal(0, 0.02, (N_KEYPOINTS, 3))).astype(np.float32)
    return scan, tgt, keys


def measure(reps, base_reps, with_baseline, only=None, kernels_only=False):
    torch.cuda.set_device(0)
    from rgc_slam_amd import _lib, features
    scan, tgt, keys = clouds()
    f = features.FPFHEstimation(0)
    L, h = f._L, f._h
    stream = L.rgc_stream(h)
    d_scan, d_map, d_keys = torch.from_numpy(scan).cuda(), torch.from_numpy(tgt).cuda(), torch.from_numpy(keys).cuda()
    normals = {}
    for which, d in (("scan", d_scan), ("map", d_map)):       # the normals stay where rgc_normal_estimate leaves them
        n4 = torch.empty((len(d), 4), dtype=torch.float32, device="cuda")
        prm, valid = _lib.NormalParams(), C.c_int(0)
        L.rgc_default_normal_params(C.byref(prm))
        prm.k = 10
        assert L.rgc_normal_estimate(h, d.data_ptr(), len(d), 12, None, 0, 0, 1, C.byref(prm), n4.data_ptr(), None, None, None, C.byref(valid)) == 0
        normals[which] = n4
    rows = []
    for wi, (name, which, radius) in enumerate(WORKLOADS):
        if only is not None and wi != only:
            continue
        d_q, d_s, d_n = (d_scan, None, normals["scan"]) if which == "scan" else (d_keys, d_map, normals["map"])
        n, ns = len(d_q), len(d_s) if d_s is not None else len(d_q)
        d_out = torch.empty((n, 33), dtype=torch.float32, device="cuda")
        d_cnt = torch.empty(n, dtype=torch.int32, device="cuda")
        valid, info, prm = C.c_int(0), _lib.FpfhInfo(), _lib.FpfhParams()
        prm.radius = radius
        call = lambda: L.rgc_fpfh_estimate(h, d_q.data_ptr(), n, 12, d_s.data_ptr() if d_s is not None else None, ns if d_s is not None else 0, 12 if d_s is not None else 0,
                                           d_n.data_ptr(), 16, 1, C.byref(prm), d_out.data_ptr(), None, None, d_cnt.data_ptr(), C.byref(valid))
        assert call() == 0
        if kernels_only:
            for _ in range(5):
                assert call() == 0
            continue
        us = timed(stream, call, reps)
        L.rgc_fpfh_get_info(h, C.byref(info))
        got = d_out.cpu().numpy()
        members = int(d_cnt.to(torch.int64).sum().item())
        run = dict(name=name, n=n, n_surface=ns, radius=radius, us=us, reps=reps, n_valid=valid.value, n_spfh=info.n_spfh, members_per_query=members / n, pairs=info.pairs,
                   pairs_per_spfh=info.pairs / max(info.n_spfh, 1), candidates=info.candidates, cell=info.cell,
                   checksum=int(np.ascontiguousarray(got).view(np.uint32).astype(np.uint64).sum()))   # (of the descriptors' bit patterns)
        if with_baseline and which == "scan":               # the same call at fixed cell sizes of the call's grid (rgc_fpfh_set_cell) beside the automatic rule's
            run["cells"] = []
            for cell in CELLS:
                assert L.rgc_fpfh_set_cell(h, cell) == 0 and call() == 0
                us_c = timed(stream, call, reps)
                L.rgc_fpfh_get_info(h, C.byref(info))
                run["cells"].append(dict(cell=cell, us=us_c, candidates=info.candidates, same_descriptors=bool(np.array_equal(np.nan_to_num(d_out.cpu().numpy()), np.nan_to_num(got)))))
            assert L.rgc_fpfh_set_cell(h, 0.0) == 0
        if with_baseline:
            run["baseline"] = baseline(L, h, stream, _lib, scan if which == "scan" else keys, d_q, None if which == "scan" else tgt, d_s, d_n, radius, got, base_reps)
        rows.append(run)
    f.close()
    return rows


def baseline(L, h, stream, _lib, q, d_q, surf, d_s, d_n, radius, got, base_reps):
    """what a caller did on the parent commit: the search index's radius rows downloaded, the normals downloaded, both passes in numpy"""
    T = q if surf is None else surf
    d_t = d_q if d_s is None else d_s
    res = {}

    def radius_rows(d_queries, nq):
        total = C.c_longlong(0)
        rc = L.rgc_search_radius(h, d_queries.data_ptr(), nq, 12, 1, radius, 0, 0, None, None, None, 0, C.byref(total))     # the size-then-fill protocol's first call
        assert rc in (0, _lib.ERR_INVALID)
        m = int(total.value)
        d_off = torch.empty(nq + 1, dtype=torch.int32, device="cuda")
        d_idx, d_sq = torch.empty(max(m, 1), dtype=torch.int32, device="cuda"), torch.empty(max(m, 1), dtype=torch.float32, device="cuda")
        assert L.rgc_search_radius(h, d_queries.data_ptr(), nq, 12, 1, radius, 0, 0, d_off.data_ptr(), d_idx.data_ptr(), d_sq.data_ptr(), m, C.byref(total)) == 0
        off, idx, sq = np.empty(nq + 1, np.int32), np.empty(m, np.int32), np.empty(m, np.float32)
        assert L.rgc_download(h, off.ctypes.data, d_off.data_ptr(), off.nbytes) == 0
        if m:
            assert L.rgc_download(h, idx.ctypes.data, d_idx.data_ptr(), idx.nbytes) == 0 and L.rgc_download(h, sq.ctypes.data, d_sq.data_ptr(), sq.nbytes) == 0
        return off.astype(np.int64), idx.astype(np.int64), sq

    def whole():
        assert L.rgc_search_set_cloud(h, d_t.data_ptr(), len(T), 12, 1, 0.0) == 0
        n4 = np.empty((len(T), 4), np.float32)
        assert L.rgc_download(h, n4.ctypes.data, d_n.data_ptr(), n4.nbytes) == 0
        off, idx, sq = radius_rows(d_q, len(q))
        if surf is None:
            counts, m = host_spfh(T, n4[:, :3], np.arange(len(T)), off, idx)
            res["bytes"] = off.nbytes // 2 + idx.nbytes // 2 + sq.nbytes + n4.nbytes
        else:                                               # the SPFHs of the members only: a second search, of the marked surface points
            marked = np.unique(idx)
            d_marked = torch.from_numpy(np.ascontiguousarray(T[marked])).cuda()
            off2, idx2, sq2 = radius_rows(d_marked, len(marked))
            part, pm = host_spfh(T, n4[:, :3], marked, off2, idx2)
            counts, m = np.zeros((len(T), 33), np.int64), np.zeros(len(T), np.int64)
            counts[marked], m[marked] = part, pm
            res["bytes"] = off.nbytes // 2 + idx.nbytes // 2 + sq.nbytes + off2.nbytes // 2 + idx2.nbytes // 2 + sq2.nbytes + n4.nbytes
        res["fpfh"] = host_fpfh(counts, m, off, idx, sq)

    us = timed(stream, whole, base_reps, warm=1)
    assert L.rgc_search_clear(h) == 0
    both = ~np.isnan(got[:, 0]) & ~np.isnan(res["fpfh"][:, 0])
    assert np.array_equal(np.isnan(got[:, 0]), np.isnan(res["fpfh"][:, 0]))
    return dict(us=us, reps=base_reps, downloaded_bytes=int(res["bytes"]), largest_difference_of_an_entry=float(np.abs(got[both] - res["fpfh"][both]).max()) if both.any() else 0.0)


def kernel_times(wi):
    """average nanoseconds per launch of every kernel of six calls of one workload (and its set-up), from a child under rocprofv3 --kernel-trace --stats"""
    with tempfile.TemporaryDirectory() as d:
        p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "fp", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), "--child",
                            "--kernels-child", str(wi)], capture_output=True, text=True, timeout=600)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if p.returncode != 0 or not files:
            return dict(error="rocprofv3 run failed (%d): %s" % (p.returncode, p.stderr[-500:]))
        out = []
        for r in csv.DictReader(open(files[0])):
            out.append(dict(kernel=r["Name"].split("(")[0], calls=int(r["Calls"]), total_ns=int(float(r["TotalDurationNs"])), average_ns=float(r["AverageNs"]), max_ns=int(float(r["MaxNs"]))))
        return sorted(out, key=lambda k: -k["total_ns"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--base-reps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--variants", default="")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--kernels-child", type=int, default=None)
    a = ap.parse_args()
    if a.child:
        rows = measure(a.reps, a.base_reps, with_baseline=not a.no_baseline, only=a.kernels_child, kernels_only=a.kernels_child is not None)
        print("ROWS " + json.dumps(rows))
        return
    variants = [("product", None)] + [(v.split("=")[0], os.path.abspath(v.split("=", 1)[1])) for v in a.variants.split(",") if v]
    runs = []
    for rnd in range(a.rounds):          # the builds alternate: other people's work shares the host
        for label, lib in variants:
            env = dict(os.environ)
            env.pop("RGC_HIP_LIB", None)
            if lib:
                env["RGC_HIP_LIB"] = lib
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--base-reps", str(a.base_reps)]
            if lib or rnd > 0:           # the baseline once, with the product
                cmd.append("--no-baseline")
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1100)
            if p.returncode != 0:
                sys.exit("the measurement of %s failed (%d):\n%s" % (label, p.returncode, p.stderr[-2000:]))
            rows = json.loads([l for l in p.stdout.splitlines() if l.startswith("ROWS ")][-1][5:])
            runs.append(dict(build=label, library="product" if not lib else os.path.basename(lib), round=rnd, rows=rows))
            print("round %d, %s: done" % (rnd, label), file=sys.stderr, flush=True)
    # every build must have computed the same thing: the counts do not depend on the group sizes (the descriptors' last bits may, with the other layout)
    for run in runs[1:]:
        assert [(x["n_valid"], x["n_spfh"], x["pairs"]) for x in runs[0]["rows"]] == [(x["n_valid"], x["n_spfh"], x["pairs"]) for x in run["rows"]]
        run["same_descriptor_bits_as_the_first_run"] = [x["checksum"] for x in runs[0]["rows"]] == [x["checksum"] for x in run["rows"]]   # (bins to lanes: expected whatever the group sizes)
    res = dict(device=torch.cuda.get_device_name(0), method="HIP events on rgc_stream(ctx) around each WHOLE call, [median, min, max] microseconds of --reps repetitions after 3 "
               "warm-up calls; a call is the normals' check, the grid build (with the box's read-back), the mark / scan / list of a separate surface, the SPFH pass, the combine pass "
               "and the read-back of the read-out words (synchronised); clouds, normals, descriptors and counts in device memory; the baseline is the route through the search "
               "index with its downloads and the two passes in numpy on the host inside the timed span, --base-reps repetitions after one warm-up; one child process per library "
               "build, the builds alternated over the rounds; kernels: average time per launch of six calls per workload under rocprofv3 --kernel-trace --stats, a child per workload",
               runs=runs)
    if a.kernels:
        res["kernels"] = [dict(name=WORKLOADS[wi][0], radius=WORKLOADS[wi][2], kernels=kernel_times(wi)) for wi in range(len(WORKLOADS))]
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
