"""FastGICP measurement: GPU time (HIP events on the context's stream, median of --reps after warm-up) of one rgc_gicp_linearize next to rgc_fitness (the same exact search and nothing else) and rgc_linearize (VGICP) on the same clouds, and of a whole rgc_gicp_align next to rgc_align, at the headline size (30 k-point scan, 1 M-point map, 1 m cells) and at the loop-closure size.  Per-kernel times: run this script under rocprofv3 --kernel-trace --stats in a run of its own.
    python scripts/bench_gicp.py --out profiles/r09_gicp.json [--reps 15]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import rgc_slam_amd.synth as synth
from rgc_slam_amd.gicp import FastGICP
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
    g = FastGICP(0)
    stream = g._L.rgc_stream(g._h)
    g.setInputTarget(tgt)
    g.setInputSource(src)
    g.synchronize()
    T = guess.astype(np.float64)
    row = dict(name=name, n_target=len(tgt), n_source=len(src), reps=reps)
    row["fitness_ms"] = timed(stream, lambda: g.fitnessAt(guess), reps)
    row["vgicp_linearize_ms"] = timed(stream, lambda: FastVGICP.linearize(g, T), reps)
    row["gicp_linearize_ms"] = timed(stream, lambda: g.linearize(T), reps)
    row["gicp_pairs"] = g.num_correspondences
    row["gicp_compute_error_ms"] = timed(stream, lambda: g.compute_error(T), reps)
    row["vgicp_align_ms"] = timed(stream, lambda: FastVGICP.align(g, guess, want_output=False), reps)
    row["vgicp_iterations"], row["vgicp_T"] = g.nr_iterations, g.getFinalTransformation().tolist()
    row["gicp_align_ms"] = timed(stream, lambda: g.align(guess, want_output=False), reps)
    row["gicp_iterations"], row["gicp_converged"], row["gicp_T"] = g.nr_iterations, bool(g.hasConverged()), g.getFinalTransformation().tolist()
    g.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=15)
    a = ap.parse_args()
    rows = []
    T_true = synth.se3(synth.rot_zyx(0.02, 0.005, -0.004), [0.2, -0.1, 0.03])
    Ti = np.linalg.inv(T_true)
    for name, nt, ns in (("headline: 30 k-point scan, 1 M-point map, 1 m cells", 1000000, 30000), ("loop closure: 20 k-point key frame, 200 k-point sub-map", 200000, 20000)):
        world, tgt = synth.make_world_and_map(nt)
        src = synth.make_scan_n(world, np.eye(4), ns)["xyz"]
        src = (src @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)
        rows.append(case(name, np.ascontiguousarray(tgt[:, :3], np.float32), src, np.eye(4, dtype=np.float32), a.reps))
    res = dict(device=torch.cuda.get_device_name(0), method="HIP events on rgc_stream(ctx) around each call, [median, min, max] ms of --reps repetitions after 3 warm-up calls; "
               "rgc_gicp_align is host-driven, so it includes its host round trips; rgc_align is the device-chained driver", rows=rows)
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
