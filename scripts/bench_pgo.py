"""Pose-graph measurement: what rgc_pgo_optimize costs on the MI355X and where the time goes, at N = 1 000 / 10 000 / 50 000 keyframes with 10 and 100
loops.  Per shape: wall time per call and per LM iteration (warm, median of --reps), the GPU time of one iteration split by kernel into edge terms,
assembly, solve and step from a rocprofv3 kernel trace of this script's own child run (--trace: needs rocprofv3), the rest being launch gaps and the
read-back, and for comparison the same damped system factored on the host by scipy's sparse LU (SuperLU, COLAMD) from a numpy assembly.
Nothing here is a pass / fail bar.     python scripts/bench_pgo.py [--reps 5] [--trace] [--shapes 1000:10,1000:100,...] [--out profiles/rNN_pgo.json]"""
import argparse, csv, glob, json, os, re, subprocess, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--trace", action="store_true")
ap.add_argument("--shapes", default="1000:10,1000:100,10000:10,10000:100,50000:10,50000:100")
ap.add_argument("--out", default=None)
ap.add_argument("--child", default=None, help="internal: N:L, one traced call")
args = ap.parse_args()
GROUPS = {"k_pgo_edges": "edge_terms", "k_pgo_gather": "assembly", "k_pgo_fold": "assembly", "k_pgo_segments": "solve", "k_pgo_dense": "solve",
          "k_pgo_backsub": "solve", "k_pgo_step": "step"}


def drive(n, n_loops, seed=7):
    """key poses of a drive that comes back on itself (a wide circle with noise) and n_loops loop edges between keyframes a lap apart, each the stored
    relative pose plus decimetres and degrees"""
    rng = np.random.default_rng(seed)
    lap = max(n // 3, 8)
    yaw = np.cumsum(2 * np.pi / lap * (1 + 0.2 * rng.standard_normal(n)))
    yaw = (yaw + np.pi) % (2 * np.pi) - np.pi
    d = 1.0 + 0.1 * rng.standard_normal(n)
    xy = np.cumsum(np.stack([d * np.cos(yaw), d * np.sin(yaw)], 1), 0)
    poses = np.stack([xy[:, 0], xy[:, 1], np.cumsum(0.02 * rng.standard_normal(n)), 0.03 * rng.standard_normal(n), 0.03 * rng.standard_normal(n), yaw], 1).astype(np.float32)
    from rgc_slam_amd import _lib
    import ctypes as C
    loops = []
    cur = np.sort(rng.choice(np.arange(lap + 1, n), n_loops, replace=False))
    for c in cur:
        l = int(c - lap + rng.integers(-3, 4))
        l = min(max(l, 0), int(c) - 2)
        a, b = poses[l].astype(np.float64), poses[int(c)].astype(np.float64)
        cy, sy = np.cos(a[5]), np.sin(a[5])
        dt = b[:3] - a[:3]
        t = np.array([cy * dt[0] + sy * dt[1], -sy * dt[0] + cy * dt[1], dt[2]]) + 0.3 * rng.standard_normal(3)     # yaw alone: an edge's error is planted anyway
        dyaw = np.rad2deg(b[5] - a[5]) + 3.0 * rng.standard_normal()
        dyaw = (dyaw + 180.0) % 360.0 - 180.0
        loops.append(_lib.PgoLoop(int(c), l, (C.c_double * 3)(*t), float(dyaw), float(np.rad2deg(a[4])), float(np.rad2deg(a[3]))))
    return poses, loops


def make_store(poses):
    from rgc_slam_amd import keyframes
    store = keyframes.KeyframeStore()
    for i, p in enumerate(poses):
        store.push(i, p)
    return store


def host_rival(store, graph, ids):
    """the first iteration's damped system assembled with numpy from the library's own read-out and solved by scipy.sparse.linalg.splu: (assembly s, solve s)"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    lin = graph.linearize(ids)
    N = len(ids)
    t0 = time.perf_counter()
    rows, cols, vals = [], [], []
    base = np.arange(4)
    def put(i, j, B):
        rows.append(np.repeat(4 * i + base, 4)); cols.append(np.tile(4 * j + base, 4)); vals.append(B.ravel())
    for n_ in range(N):
        put(n_, n_, lin["H_diag"][n_])
    for e, (i, j) in enumerate(lin["edge_ij"]):
        B = lin["H_chain"][e] if e < N - 1 else lin["H_loop"][e - (N - 1)]
        put(int(i), int(j), B); put(int(j), int(i), B.T)
    H = sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(4 * N, 4 * N))
    dg = H.diagonal()
    fixed = np.flatnonzero(dg == 0)
    H = H + sp.diags(np.clip(dg, 1e-6, 1e32) / 1e4 + np.where(dg == 0, 1.0, 0.0))
    t1 = time.perf_counter()
    d = spl.splu(H.tocsc()).solve(-lin["g"].ravel())
    t2 = time.perf_counter()
    assert len(fixed) == 4 and np.all(d[fixed] == 0)
    return t1 - t0, t2 - t1


def child(shape):
    n, nl = [int(v) for v in shape.split(":")]
    from rgc_slam_amd import pose_graph
    poses, loops = drive(n, nl)
    store = make_store(poses)
    g = pose_graph.PoseGraph4DoF(store)
    g.loops = loops
    rep, _ = g.optimize(list(range(n)), apply=False)
    print("CHILD", json.dumps(rep))
    store.close()


def traced(shape):
    """kernel time of one rgc_pgo_optimize by group, from rocprofv3 --kernel-trace over a child run of this script"""
    with tempfile.TemporaryDirectory() as td:
        r = subprocess.run(["rocprofv3", "--kernel-trace", "-d", td, "-o", "pgo", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), "--child", shape],
                           capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            return {"error": (r.stderr or r.stdout)[-400:]}
        rep = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("CHILD ")][0][6:])
        out = {k: 0.0 for k in set(GROUPS.values())}
        per = {}
        for f in glob.glob(os.path.join(td, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                name = re.sub(r"\(.*", "", row["Kernel_Name"]).split("::")[-1].replace(".kd", "")
                if name in GROUPS:
                    ms = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-6
                    out[GROUPS[name]] += ms
                    per[name] = per.get(name, 0.0) + ms
        evals = rep["iterations"] + 1
        return {"iterations": rep["iterations"], "evaluations": evals, "gpu_ms_total_by_group": out, "gpu_ms_total_by_kernel": per,
                "gpu_ms_per_iteration": {k: (v / max(rep["iterations"], 1)) for k, v in out.items()}}


def main():
    if args.child:
        return child(args.child)
    from rgc_slam_amd import pose_graph
    res = {"what": "rgc_pgo_optimize: wall ms per call and per LM iteration (median of %d warm calls), GPU ms by kernel group from a rocprofv3 kernel trace of "
                   "one call, and the first iteration's system on the host (numpy assembly from the read-out + scipy splu)" % args.reps, "shapes": []}
    for shape in args.shapes.split(","):
        n, nl = [int(v) for v in shape.split(":")]
        poses, loops = drive(n, nl)
        store = make_store(poses)
        g = pose_graph.PoseGraph4DoF(store)
        g.loops = loops
        ids = list(range(n))
        rep, _ = g.optimize(ids, apply=False)          # warm: buffers allocated
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            rep, _ = g.optimize(ids, apply=False)
            ts.append(time.perf_counter() - t0)
        row = {"n_keyframes": n, "n_loops": nl, "report": rep, "wall_ms_per_call": 1e3 * float(np.median(ts)),
               "wall_ms_per_iteration": 1e3 * float(np.median(ts)) / max(rep["iterations"], 1)}
        try:
            a, s = host_rival(store, g, ids)
            row["host_scipy_splu_ms"] = {"assembly": 1e3 * a, "factor_and_solve": 1e3 * s}
        except Exception as e:   # noqa: BLE001  (scipy is optional)
            row["host_scipy_splu_ms"] = {"error": str(e)}
        store.close()
        if args.trace:
            row["trace"] = traced(shape)
            if "gpu_ms_per_iteration" in row["trace"]:
                row["wall_minus_gpu_ms_per_iteration"] = row["wall_ms_per_iteration"] - sum(row["trace"]["gpu_ms_per_iteration"].values())
        print(json.dumps(row))
        res["shapes"].append(row)
    out = args.out
    if out is None:
        nums = [int(m.group(1)) for m in (re.match(r"r(\d+)_", f) for f in os.listdir(os.path.join(ROOT, "profiles"))) if m]
        out = os.path.join(ROOT, "profiles", "r%02d_pgo.json" % (max(nums) + 1))
    json.dump(res, open(out, "w"), indent=1)
    print("wrote", out)


main()
