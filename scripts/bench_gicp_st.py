"""FastGICPSingleThread measurement: along the pose trajectory of one recorded solve (the LM driver of rgc_gicpst_align restated on the host over rgc_gicpst_linearize / rgc_gicpst_compute_error), per linearisation the searched fraction, the GPU time (HIP events on the context's stream, median of --reps passes after warm-up passes) of rgc_gicpst_linearize from a reset at the first pose on, and of rgc_gicp_linearize at the same pose in the same process (the two alternate pass by pass); then whole rgc_gicpst_align and rgc_gicp_align solves.  At the headline size (30 k-point scan, 1 M-point map, 1 m cells) and the loop-closure size of scripts/bench_gicp.py.
    python scripts/bench_gicp_st.py --out profiles/r19_gicp_st.json [--reps 9]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import rgc_slam_amd.synth as synth
from rgc_slam_amd.gicp import FastGICP, FastGICPSingleThread


def so3_exp(w):
    th = float(np.linalg.norm(w))
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K


def record_solve(g, guess):
    """LsqRegistration's LM loop (lsq_registration_impl.hpp:53-172) on the host over the product's calls: returns the pose of every linearisation"""
    p = g._p
    x0, lam, poses, conv = guess.astype(np.float64).copy(), -1.0, [], False
    g.reset()
    for _ in range(p.max_iterations):
        if conv:
            break
        poses.append(x0.copy())
        y0, H, b = g.linearize(x0)
        if lam < 0:
            lam = p.lm_init_lambda_factor * np.abs(np.diag(H)).max()
        nu, ok, delta = 2.0, False, np.eye(4)
        for _ in range(p.lm_max_iterations):
            d = np.linalg.solve(H + lam * np.eye(6), -b)
            delta = np.eye(4)
            delta[:3, :3], delta[:3, 3] = so3_exp(d[:3]), d[3:]
            xi = delta @ x0
            rho = (y0 - g.compute_error(xi)) / float(d @ (lam * d - b))
            small = max(np.abs(delta[:3, :3] - np.eye(3)).max() / p.rotation_eps, np.abs(delta[:3, 3]).max() / p.translation_eps) < 1
            if rho < 0:
                if small:
                    ok = True
                    break
                lam, nu = nu * lam, 2 * nu
                continue
            x0, lam, ok = xi, lam * max(1.0 / 3.0, 1 - (2 * rho - 1) ** 3), True
            break
        if not ok:
            break
        conv = max(np.abs(delta[:3, :3] - np.eye(3)).max() / p.rotation_eps, np.abs(delta[:3, 3]).max() / p.translation_eps) < 1
    return poses


def event_ms(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def stats(v):
    return [float(np.median(v)), float(np.min(v)), float(np.max(v))]


def case(name, tgt, src, guess, reps, warm=2):
    g = FastGICPSingleThread(0)
    stream = torch.cuda.ExternalStream(g._L.rgc_stream(g._h))
    g.setInputTarget(tgt)
    g.setInputSource(src)
    g.synchronize()
    poses = record_solve(g, guess)
    st_ms, plain_ms, searched = [[] for _ in poses], [[] for _ in poses], [0] * len(poses)
    for r in range(warm + reps):
        g.reset()
        for i, T in enumerate(poses):                      # the cached route: a reset, then the whole trajectory in order
            t = event_ms(stream, lambda: g.linearize(T))
            searched[i] = g.num_searched()
            if r >= warm:
                st_ms[i].append(t)
        for i, T in enumerate(poses):                      # FastGICP at the same poses: a full exact search each time
            t = event_ms(stream, lambda: FastGICP.linearize(g, T))
            if r >= warm:
                plain_ms[i].append(t)
    row = dict(name=name, n_target=len(tgt), n_source=len(src), reps=reps, linearisations=len(poses),
               per_linearisation=[dict(i=i, searched=searched[i], searched_fraction=searched[i] / len(src), gicpst_linearize_ms=stats(st_ms[i]),
                                       gicp_linearize_ms=stats(plain_ms[i])) for i in range(len(poses))])
    st_solve, plain_solve = [], []
    for r in range(warm + reps):
        a = event_ms(stream, lambda: g.align(guess, want_output=False))
        it_st, conv_st, T_st = g.nr_iterations, bool(g.hasConverged()), g.getFinalTransformation().tolist()
        b = event_ms(stream, lambda: FastGICP.align(g, guess, want_output=False))
        it_pl, conv_pl, T_pl = g.nr_iterations, bool(g.hasConverged()), g.getFinalTransformation().tolist()
        if r >= warm:
            st_solve.append(a)
            plain_solve.append(b)
    row.update(gicpst_align_ms=stats(st_solve), gicpst_iterations=it_st, gicpst_converged=conv_st, gicpst_T=T_st,
               gicp_align_ms=stats(plain_solve), gicp_iterations=it_pl, gicp_converged=conv_pl, gicp_T=T_pl)
    g.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    rows = []
    T_true = synth.se3(synth.rot_zyx(0.02, 0.005, -0.004), [0.2, -0.1, 0.03])
    Ti = np.linalg.inv(T_true)
    for name, nt, ns in (("headline: 30 k-point scan, 1 M-point map, 1 m cells", 1000000, 30000), ("loop closure: 20 k-point key frame, 200 k-point sub-map", 200000, 20000)):
        world, tgt = synth.make_world_and_map(nt)
        src = synth.make_scan_n(world, np.eye(4), ns)["xyz"]
        src = (src @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)
        rows.append(case(name, np.ascontiguousarray(tgt[:, :3], np.float32), src, np.eye(4, dtype=np.float32), a.reps))
    res = dict(device=torch.cuda.get_device_name(0), method="HIP events on rgc_stream(ctx) around each call (each ends in a stream synchronise), [median, min, max] ms of --reps passes "
               "after 2 warm-up passes; a pass = rgc_gicpst_reset, then rgc_gicpst_linearize at every pose of the recorded solve in order, then rgc_gicp_linearize at the same poses; "
               "both solves are host-driven and include their host round trips", rows=rows)
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
