"""RBF covariance estimation measured: GPU time of preparing the target and the source at c1 size (30 k-point scan, 1 M-point map, 1 m cells) under
RGC_COV_RBF at the defaults 0.5 / 3.0 and at 0.25 / 1.25, next to the kNN general route (k_knn_cov6) and the tuned route on the same clouds.  Two clocks:
HIP events on the context's streams around the whole preparation (rgc_set_target_device / rgc_set_source_device; [median, min, max] of --reps after
warm-up), and the library's own event pairs around the covariance launch alone (rgc_profile_*, kinds knn_cov_target / knn_cov_source).  Mean ball size from an fp64
cKDTree on a sample of the points; pairs/s = points x mean ball / covariance time; the fp64 share counts the 23 fp64 operations the moment spends per
member (1 for the exponent, 3 differences, 9 products, 10 additions: exp itself is NOT counted) against the data sheet's 78.6 TFLOP/s vector fp64.
    python scripts/bench_rbf.py --out profiles/r10_rbf.json [--reps 7] [--n-target 1000000]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from scipy.spatial import cKDTree

import rgc_slam_amd.synth as synth
from rgc_slam_amd.registration import FastVGICP

FP64_VECTOR_TFLOPS = 78.6
FLOPS_PER_MEMBER = 23


def stats(x):
    return [float(np.median(x)), float(np.min(x)), float(np.max(x))]


def mean_ball(P, max_dist, sample=2000):
    rng = np.random.default_rng(0)
    q = P[rng.choice(len(P), min(sample, len(P)), replace=False)].astype(np.float64)
    return float(np.mean(cKDTree(P.astype(np.float64)).query_ball_point(q, max_dist, return_length=True)))


def run(label, tgt4, src4, configure, reps, warm=2):
    v = FastVGICP(0)
    v.setResolution(1.0)
    configure(v)
    dt, ds = v.device_alloc(tgt4.nbytes), v.device_alloc(src4.nbytes)
    v.upload(dt, tgt4); v.upload(ds, src4)
    s_main = torch.cuda.ExternalStream(v._L.rgc_stream(v._h))
    v.profile_enable(True)
    row = dict(route=label)
    for what, ptr, n, setter, kind in (("target", dt, len(tgt4), v.setInputTargetDevice, "knn_cov_target"), ("source", ds, len(src4), v.setInputSourceDevice, "knn_cov_source")):
        whole, cov = [], []
        for i in range(warm + reps):
            v.synchronize()
            v.profile_reset()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s_main)
            setter(ptr, n, 16)
            v.synchronize()                       # (the source is prepared on the context's second stream: the host waits for both)
            b.record(s_main)
            b.synchronize()
            if i >= warm:
                whole.append(a.elapsed_time(b))
                p = v.profile()
                cov.append(sum(r["total_ms"] for name, r in p.items() if name == kind))
        row[what + "_prepare_ms"] = stats(whole)
        row[what + "_covariance_ms"] = stats(cov)
    v.device_free(dt); v.device_free(ds)
    v.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--n-target", type=int, default=1000000)
    ap.add_argument("--n-source", type=int, default=30000)
    a = ap.parse_args()
    world, tgt = synth.make_world_and_map(a.n_target)
    src = synth.make_scan_n(world, np.eye(4), a.n_source)["xyz"]
    tgt4 = np.zeros((len(tgt), 4), np.float32); tgt4[:, :3] = tgt[:, :3]
    src4 = np.zeros((len(src), 4), np.float32); src4[:, :3] = src[:, :3]
    rows = []
    rows.append(run("tuned (PLANE, kNN k = 20)", tgt4, src4, lambda v: None, a.reps))
    rows.append(run("general, kNN k = 20 (k_knn_cov6, MIN_EIG)", tgt4, src4, lambda v: v.setRegularizationMethod(v.REG_MIN_EIG), a.reps))
    for kw, md in ((0.25, 1.25), (0.5, 3.0)):
        def conf(v, kw=kw, md=md):
            v.setRegularizationMethod(v.REG_MIN_EIG)
            v.setNearestNeighborSearchMethod(v.NearestNeighborMethod.GPU_RBF_KERNEL)
            v.setKernelWidth(kw, md)
        r = run(f"general, RBF {kw} / {md} (k_rbf_cov6, MIN_EIG)", tgt4, src4, conf, a.reps)
        for what, P in (("target", tgt4[:, :3]), ("source", src4[:, :3])):
            mb = mean_ball(P, md)
            ms = r[what + "_covariance_ms"][0]
            pairs = len(P) * mb
            r[what + "_mean_ball"] = mb
            r[what + "_pairs_per_s"] = pairs / (ms * 1e-3) if ms > 0 else None
            r[what + "_fp64_share"] = pairs * FLOPS_PER_MEMBER / (ms * 1e-3) / (FP64_VECTOR_TFLOPS * 1e12) if ms > 0 else None
        rows.append(r)
    res = dict(device=torch.cuda.get_device_name(0), n_target=len(tgt4), n_source=len(src4), reps=a.reps,
               method="[median, min, max] ms; *_prepare_ms: HIP events on rgc_stream(ctx) around rgc_set_*_device + rgc_synchronize (grid build, covariances, voxel map; "
                      "includes the host's enqueue); *_covariance_ms: the library's event pair around the covariance launch alone (rgc_profile_get); mean ball: fp64 "
                      "cKDTree on 2000 sampled points; fp64 share: 23 operations per member (exp not counted) against 78.6 TFLOP/s",
               rows=rows)
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
