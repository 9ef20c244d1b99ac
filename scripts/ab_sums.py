"""The sums of every solver that shares csrc/rgc_terms.h, as bits: runs the linearise-type calls of each method on the designed cases the tests
build (tests/gicp_mp_cases.py, tests/mapreg_cases.py, tests/fe_cases.py, the scenes of tests/test_gpu_gicp.py, tests/test_gpu_ndt.py and
tests/test_gpu_voxel_lookup.py) and prints one line per case: a SHA-256 of the returned cost, H and b bytes.  Two builds of the library compute the
same sums bit for bit iff the two lists are equal:
    RGC_HIP_LIB=<build A> python scripts/ab_sums.py > a.txt;  RGC_HIP_LIB=<build B> python scripts/ab_sums.py > b.txt;  diff a.txt b.txt
(one process per build: a process loads one library).  Needs a GPU."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def digest(*parts):
    h = hashlib.sha256()
    for p in parts:
        h.update(np.ascontiguousarray(np.asarray(p, dtype=np.float64)).tobytes())
    return h.hexdigest()[:32]


def line(name, *parts):
    print("%-58s %s" % (name, digest(*parts)), flush=True)


def terms_of(g, T, T3):
    """cost, H, b at T, the cost alone (want_H off), and the frozen cost at T3"""
    y, H, b = g.linearize(T)
    y0 = g.linearize(T, want_H=False)[0]
    return y, H, b, y0, g.compute_error(T3)


def run_gicp():
    import gicp_mp_cases as mc
    import ndt_reference as nr
    from rgc_slam_amd import gicp, registration
    d = mc.scene_data()                              # tests/test_gpu_gicp.py's scene, call for call (plus 200 far source points)
    d3 = np.array([0.002, -0.001, 0.003, 0.01, -0.02, 0.015])
    for label, nt, ns, k, method in (("plane_k20", 24000, 8200, 20, None), ("plane_k2", 24000, 8200, 2, None),
                                     ("min_eig_k10", 12000, 3000, 10, registration.FastVGICP.REG_MIN_EIG),
                                     ("frobenius_k20", 12000, 3000, 20, registration.FastVGICP.REG_FROBENIUS)):
        g = gicp.FastGICP(0)
        g.setCorrespondenceRandomness(k)
        if method is not None:
            g.setRegularizationMethod(method)
        g.setInputTarget(d["tgt"][:nt])
        g.setInputSource(d["src"][:ns])
        for p, T in enumerate(d["poses"][:3]):
            line("gicp %s pose %d" % (label, p), *terms_of(g, T, nr.increment(d3, T)[0]))
        g.close()


def run_gicp_mp():
    import gicp_mp_cases as mc
    from rgc_slam_amd import gicp
    for case in mc.all_cases():
        g = gicp.FastGICPMultiPoints(0)
        g.setCorrespondenceRandomness(case.get("k", 2 if min(len(case["tgt"]), len(case["src"])) < 20 else 20))
        g.setNeighborSearchRadius(case["r"])
        g.setInputTarget(case["tgt"])
        g.setInputSource(case["src"])
        for p, T in enumerate(case["poses"]):
            y, H, b = g.linearize(T)
            line("gicpmp %s pose %d" % (case["name"], p), y, H, b, g.linearize(T, want_H=False)[0], g.num_correspondences, g.num_pairs)
        g.close()


def run_ndt():
    import ndt_reference as nr
    from rgc_slam_amd import ndt
    rng = np.random.default_rng(9001)                # tests/test_gpu_ndt.py's scene (before its points near a voxel wall are redrawn)
    tgt = nr.scene(rng, 24000)
    T = nr.random_pose(rng, about=(100.0, -60.0, 2.0))
    Ti = np.linalg.inv(T)
    src = (nr.scene(rng, 8000).astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3] + rng.normal(0, 0.01, (8000, 3))).astype(np.float32)
    d3 = np.array([0.002, -0.001, 0.003, 0.01, -0.02, 0.015])
    for mode in (nr.P2D, nr.D2D):
        for method, radius in ((nr.DIRECT1, 0.0), (nr.DIRECT7, 0.0), (nr.DIRECT27, 0.0), (nr.DIRECT_RADIUS, 1.5)):
            for res in (0.5, 1.0):
                r = ndt.NDTRegistration()
                r.setResolution(res)
                r.setDistanceMode(mode)
                r.setNeighborSearchMethod(method, radius)
                r.setInputTarget(tgt)
                r.setInputSource(src)
                for p, P in enumerate((T, np.eye(4))):
                    line("ndt mode %d method %d res %.1f pose %d" % (mode, method, res, p), *terms_of(r, P, nr.increment(d3, P)[0]), r.num_correspondences())
                r.close()


def run_vgicp():
    import rgc_slam_amd.synth as synth
    from rgc_slam_amd import registration
    world, tgt = synth.make_world_and_map(30000, seed=synth.SEED + 61)      # tests/test_gpu_voxel_lookup.py's clouds and poses
    T_true = synth.se3(synth.rot_zyx(0.012, 0.002, -0.001), [0.11, 0.03, 0.002])
    src = synth.make_scan_n(world, T_true, 8000, seed=synth.SEED + 61)["xyz"]
    big = synth.make_scan_n(world, T_true, 40000, seed=synth.SEED + 62)["xyz"]
    T_lin = synth.se3(synth.rot_zyx(0.015, -0.004, 0.003), [0.09, 0.05, -0.01])
    T_err = synth.se3(synth.rot_zyx(0.0155, -0.0041, 0.0028), [0.094, 0.046, -0.012])
    for route in ("tuned", "general"):
        for res in (0.3, 1.0):
            if route == "general":
                os.environ["RGC_FORCE_GENERAL"] = "1"
            v = registration.odometer_vgicp(0)
            os.environ.pop("RGC_FORCE_GENERAL", None)
            v.setResolution(res)
            if route == "general":
                v.setRegularizationMethod(registration.FastVGICP.REG_MIN_EIG)
                v.setVoxelAccumulationMode(registration.FastVGICP.VOXEL_MULTIPLICATIVE)
            v.setInputTarget(tgt)
            for sname, s in (("8k", src), ("40k", big)):
                v.setInputSource(s)
                for method, code in (("DIRECT27", 0), ("DIRECT7", 1), ("DIRECT1", 2)):
                    v.setNeighborSearchMethod(code)
                    cost, H, b = v.linearize(T_lin)
                    line("vgicp %s res %.1f %s %s" % (route, res, sname, method), cost, H, b, v.compute_error(T_err))
            v.close()


def run_mapreg():
    import mapreg_cases as mc
    from rgc_slam_amd import mapping
    r = mapping.MapFeatureRegistration(0)
    r.setInputMaps(*mc.maps())
    for name in list(mc.SPECS) + list(mc.SHAPE_SPECS):
        c = mc.build(name)
        f = c["feat"]
        for label, x_eval in (("x0", None), ("x_eval", c["x_eval"])):
            o = r.linearize(f[0], f[1], f[2], f[3], c["x0"], x_eval, ground_cur=c["ground"][0], ground_last=c["ground"][1], imu=c["imu"], want_factors=False)
            line("mapreg %s %s" % (name, label), o["cost"], o["H"], o["g"], o["n_factors"])
    r.close()


def run_frontend():
    import fe_cases
    from rgc_slam_amd import frontend
    fe = frontend.ScanRegistration(16)
    for name, c in fe_cases.CASES.items():
        if c.refused:
            continue
        raw, prm, _ = fe_cases.get(name)
        fe.params.n_scans, fe.params.use_intensity = prm["n_scans"], prm.get("use_intensity", 1)
        g = fe.laserCloudHandler(raw)
        line("frontend %s" % name, g["groundparam"], g["n_ground"], int(bool(g["ground_valid"])))
    fe.close()


if __name__ == "__main__":
    which = sys.argv[1:] or ["gicp", "gicp_mp", "ndt", "vgicp", "mapreg", "frontend"]
    for w in which:
        globals()["run_" + w]()
