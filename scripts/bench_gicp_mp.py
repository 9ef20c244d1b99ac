"""FastGICPMultiPoints measurement: GPU time (HIP events on the context's stream, median of --reps after warm-up) of one rgc_gicpmp_linearize -- the exact radius gather and merge, then the terms -- at radii 0.25, 0.5 and 1.0, next to rgc_gicp_linearize (one exact nearest neighbour per point) on the same clouds, with the candidates and the pairs per query beside them, at the headline size (30 k-point scan, 1 M-point map, 1 m cells) and at c1 size (30 k / 100 k).  --variants G=LIB[,G=LIB ...]: the same measurement in a child process per developer build of the library with another lane-group size (RGC_EXTRA_FLAGS=-DRGC_LAB_MP_GROUP=G RGC_LIB_OUT=LIB python rgc-slam_amd/build.py), alternated with the product over --rounds rounds.
    python scripts/bench_gicp_mp.py --out profiles/r18_gicp_mp.json [--reps 15] [--variants 1=/tmp/g1.so,8=/tmp/g8.so,64=/tmp/g64.so]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

RADII = (0.25, 0.5, 1.0)
SIZES = (("headline: 30 k-point scan, 1 M-point map, 1 m cells", 1000000, 30000), ("c1 size: 30 k-point scan, 100 k-point map", 100000, 30000))
PRODUCT_GROUP = 8   # rgck::MP_GROUP of csrc/rgc_gicp_mp.hip


def timed(stream, fn, reps, warm=3):
    """[median, min, max] GPU milliseconds between two events recorded on `stream` around fn()"""
    s = torch.cuda.ExternalStream(stream, device=torch.device("cuda", 0))
    out = []
    for i in range(warm + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        fn()
        b.record(s)
        b.synchronize()
        if i >= warm:
            out.append(a.elapsed_time(b))
    return [float(np.median(out)), float(np.min(out)), float(np.max(out))]


def measure(reps, with_gicp):
    """the rows of this process's library"""
    torch.cuda.set_device(0)
    import rgc_slam_amd.synth as synth
    from rgc_slam_amd.gicp import FastGICP, FastGICPMultiPoints
    T_true = synth.se3(synth.rot_zyx(0.02, 0.005, -0.004), [0.2, -0.1, 0.03])
    Ti = np.linalg.inv(T_true)
    rows = []
    for name, nt, ns in SIZES:
        world, tgt = synth.make_world_and_map(nt)
        src = synth.make_scan_n(world, np.eye(4), ns)["xyz"]
        src = (src @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)
        tgt = np.ascontiguousarray(tgt[:, :3], np.float32)
        g = FastGICPMultiPoints(0)
        stream = g._L.rgc_stream(g._h)
        g.setInputTarget(tgt)
        g.setInputSource(src)
        g.synchronize()
        T = np.eye(4)
        row = dict(name=name, n_target=len(tgt), n_source=len(src), reps=reps, radii=[])
        if with_gicp:
            row["gicp_linearize_ms"] = timed(stream, lambda: FastGICP.linearize(g, T), reps)
        for r in RADII:
            g.setNeighborSearchRadius(r)
            ms = timed(stream, lambda: g.linearize(T), reps)
            cost = g.linearize(T, want_H=False)[0]
            row["radii"].append(dict(radius=r, linearize_ms=ms, points_with_a_neighbour=g.num_correspondences, pairs_per_query=g.num_pairs / len(src),
                                     candidates_per_query=g.num_candidates / len(src), cost=cost))
        g.close()
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--variants", default="")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        print("ROWS " + json.dumps(measure(a.reps, with_gicp=not os.environ.get("RGC_HIP_LIB"))))
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
    # every build must have computed the same thing: the same pairs, candidates and (to the order of its sums) cost
    base = runs[0]["rows"]
    for run in runs[1:]:
        for r0, r1 in zip(base, run["rows"]):
            for a0, a1 in zip(r0["radii"], r1["radii"]):
                assert (a0["points_with_a_neighbour"], a0["pairs_per_query"], a0["candidates_per_query"]) == (a1["points_with_a_neighbour"], a1["pairs_per_query"], a1["candidates_per_query"])
                assert abs(a0["cost"] - a1["cost"]) <= 1e-9 * abs(a0["cost"]), (a0["cost"], a1["cost"])
    res = dict(device=torch.cuda.get_device_name(0), method="HIP events on rgc_stream(ctx) around each call, [median, min, max] ms of --reps repetitions after 3 warm-up calls; a call is "
               "the launches of one linearisation and its 30-double read-back (synchronised); one child process per library build, the builds alternated over the rounds", runs=runs)
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
