"""NDT measurement: GPU time (HIP events on the context's stream, median of --reps after warm-up) of the target's voxel-map build, one linearize and a whole align of the NDT registration (rgc_ndt_*) for P2D and D2D x DIRECT1 / DIRECT7 / RADIUS(1.5), at the headline size (30 k-point scan, 1 M-point map, 1 m voxels) and at the loop-closure size, next to the same context's VGICP set_target + align on the same clouds.
    python scripts/bench_ndt.py --out profiles/r08_ndt.json [--reps 15]"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import rgc_slam_amd.synth as synth
from rgc_slam_amd import ndt as ndtm
from rgc_slam_amd.registration import FastVGICP


def timed(stream, fn, reps, warm=3):
    """median GPU milliseconds between two events recorded on `stream` around fn() (which ends synchronised or not: the second event waits)"""
    s = torch.cuda.ExternalStream(stream)
    out = []
    for i in range(warm + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        fn()
        b.record(s)
        b.synchronize()
        if i >= warm:
            out.append(a.elapsed_time(b))
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def case(name, tgt, src, guess, reps):
    v = FastVGICP(0)
    r = ndtm.NDTRegistration(owner=v)
    stream = v._L.rgc_stream(v._h)
    T = np.eye(4)
    row = dict(name=name, n_target=len(tgt), n_source=len(src), reps=reps)

    def vg_target():
        v.setInputTarget(tgt)
        v.synchronize()
    def vg_align():
        v.align(guess, want_output=False)
    v.setInputSource(src)
    row["vgicp_set_target_ms"] = timed(stream, vg_target, reps)
    row["vgicp_align_ms"] = timed(stream, vg_align, reps)
    row["vgicp_iterations"] = v.nr_iterations
    r.setInputSource(src)

    def ndt_target():
        r.setInputTarget(tgt)
        r._L.rgc_ndt_get_voxels(r._h, 0, 0, None, None, None, None, cnt)   # builds the map, reads nothing back
    cnt = C.c_int(0)
    row["ndt_target_build_ms"] = timed(stream, ndt_target, reps)
    row["ndt_target_voxels"] = cnt.value
    for mode, mname in ((ndtm.NDT_P2D, "p2d"), (ndtm.NDT_D2D, "d2d")):
        for meth, rad, hname in ((ndtm.NDT_DIRECT1, 0.0, "direct1"), (ndtm.NDT_DIRECT7, 0.0, "direct7"), (ndtm.NDT_DIRECT_RADIUS, 1.5, "radius1.5")):
            r.setDistanceMode(mode)
            r.setNeighborSearchMethod(meth, rad)
            r.linearize(T)
            key = "%s_%s" % (mname, hname)
            row[key + "_linearize_ms"] = timed(stream, lambda: r.linearize(guess), reps)
            row[key + "_terms"] = r.num_correspondences()
            row[key + "_align_ms"] = timed(stream, lambda: r.align(guess), reps)
            row[key + "_iterations"] = r.iterations()
            row[key + "_converged"] = bool(r.hasConverged())
    r.close()
    v.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=15)
    a = ap.parse_args()
    rows = []
    T_true = synth.se3(synth.rot_zyx(0.02, 0.005, -0.004), [0.2, -0.1, 0.03])
    Ti = np.linalg.inv(T_true)
    for name, nt, ns in (("headline: 30 k-point scan, 1 M-point map, 1 m voxels", 1000000, 30000), ("loop closure: 20 k-point key frame, 200 k-point sub-map", 200000, 20000)):
        world, tgt = synth.make_world_and_map(nt)
        src = synth.make_scan_n(world, np.eye(4), ns)["xyz"]
        src = (src @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)
        rows.append(case(name, np.ascontiguousarray(tgt[:, :3], np.float32), src, np.eye(4, dtype=np.float32), a.reps))
    res = dict(device=torch.cuda.get_device_name(0), method="HIP events on rgc_stream(ctx) around each call, [median, min, max] ms of --reps repetitions after 3 warm-up calls; host-driven LM, so an align includes its host round trips", rows=rows)
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
