"""VGICP DIRECT_RADIUS measurement: GPU time (HIP events on the context's stream, median of --reps after warm-up) of one rgc_linearize and host time (a clock around the call, which ends in a synchronisation) of one whole rgc_align at radii 1.5, 2.0 and 3.0 (19, 33 and 123 offsets), next to DIRECT27 on the same clouds and the same build, with a 30 k-point scan on the 1 M-point map and on the c1 map (100 k points).  --variants G=LIB[,G=LIB ...]: the same measurement in a child process per developer build of the library with another number of lanes per source point (RGC_EXTRA_FLAGS=-DRGC_LAB_VR_GROUP=G RGC_LIB_OUT=LIB python rgc-slam_amd/build.py), alternated with the product over --rounds rounds.
    python scripts/bench_vgicp_radius.py --out profiles/r20_vgicp_radius.json [--reps 15] [--variants 1=/tmp/g1.so,8=/tmp/g8.so,16=/tmp/g16.so]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

RADII = (1.5, 2.0, 3.0)
SIZES = (("headline: 30 k-point scan, 1 M-point map, 1 m cells", 1000000, 30000), ("c1 size: 30 k-point scan, 100 k-point map", 100000, 30000))
PRODUCT_GROUP = 4   # rgck::VR_GROUP of csrc/rgc_vgicp_radius.hip
FROZEN_BYTES = 52   # per source point and offset: the voxel id (4) and the six doubles of its Mahalanobis matrix


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


def walled(fn, reps, warm=2):
    """[median, min, max] host milliseconds of fn(), a call that returns after its last synchronisation"""
    out = []
    for i in range(warm + reps):
        t0 = time.perf_counter()
        fn()
        if i >= warm:
            out.append(1e3 * (time.perf_counter() - t0))
    return [float(np.median(out)), float(np.min(out)), float(np.max(out))]


def measure(reps):
    """the rows of this process's library"""
    torch.cuda.set_device(0)
    import rgc_slam_amd.synth as synth
    from rgc_slam_amd import registration
    T_true = synth.se3(synth.rot_zyx(0.02, 0.005, -0.004), [0.2, -0.1, 0.03])
    Ti = np.linalg.inv(T_true)
    I4 = np.eye(4, dtype=np.float32)
    rows = []
    for name, nt, ns in SIZES:
        world, tgt = synth.make_world_and_map(nt)
        src = synth.make_scan_n(world, np.eye(4), ns)["xyz"]
        src = (src @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)
        tgt = np.ascontiguousarray(tgt[:, :3], np.float32)
        v = registration.odometer_vgicp(0)
        stream = v._L.rgc_stream(v._h)
        v.setInputTarget(tgt)
        v.setInputSource(src)
        v.synchronize()
        row = dict(name=name, n_target=len(tgt), n_source=len(src), reps=reps, methods=[])
        for label, method, radius in [("DIRECT27", registration.DIRECT27, -1.0)] + [("DIRECT_RADIUS %.1f" % r, registration.DIRECT_RADIUS, r) for r in RADII]:
            v.setNeighborSearchMethod(method, radius)
            noff = len(registration.FastVGICP.neighbor_offsets(method, radius))
            lin = timed(stream, lambda: v.linearize(np.eye(4)), reps)
            cost = v.linearize(np.eye(4))[0]
            ncorr = v.num_correspondences
            solve = walled(lambda: v.align(I4, want_output=False), max(3, reps // 3))
            row["methods"].append(dict(method=label, offsets=noff, linearize_ms=lin, align_ms=solve, iterations=v.nr_iterations, correspondences=ncorr, cost=cost,
                                       final_T=[float(x) for x in v.getFinalTransformation().reshape(16)],
                                       frozen_bytes_per_source_point=FROZEN_BYTES * noff))
        v.close()
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
        print("ROWS " + json.dumps(measure(a.reps)))
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
            runs.append(dict(lanes_per_point=group, library="product" if not lib else os.path.basename(lib), round=rnd, rows=rows))
            print("lanes per point %d, round %d: done" % (group, rnd), file=sys.stderr, flush=True)
    # every build must have computed the same thing: the same correspondences, the cost to the order of its sums
    base = runs[0]["rows"]
    for run in runs[1:]:
        for r0, r1 in zip(base, run["rows"]):
            for a0, a1 in zip(r0["methods"], r1["methods"]):
                assert a0["correspondences"] == a1["correspondences"], (a0["method"], run["lanes_per_point"])
                assert abs(a0["cost"] - a1["cost"]) <= 1e-9 * abs(a0["cost"]), (a0["cost"], a1["cost"])
    res = dict(device=torch.cuda.get_device_name(0), method="linearize_ms: HIP events on rgc_stream(ctx) around each rgc_linearize (its launches and the 28-double read-back, "
               "synchronised), [median, min, max] ms of --reps repetitions after 3 warm-up calls; align_ms: a host clock around rgc_align from the identity guess (the host LM loop: one "
               "enqueue and one synchronised read-back per outer iteration; DIRECT27: the device LM), [median, min, max] ms of reps / 3 repetitions after 2 warm-up calls; one child process "
               "per library build, the builds alternated over the rounds", runs=runs)
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
