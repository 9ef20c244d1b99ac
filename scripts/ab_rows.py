"""Time per call of the touched entry points on the parent's and on the new library (RGC_HIP_LIB), one child process per run, both arms treated alike:
the touched rows of tests/one_context_ops.py at their large size in each form, on one context; wall-clock around the whole row (it returns behind its host
waits), the median of REPS repetitions after WARM warm-up calls.  Rounds alternate the order of the two libraries.
    python scripts/ab_rows.py ROUNDS OUT.json PARENT_LIB [NEW_LIB]"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = ["voxelgrid", "voxelgrid_in_halves", "uniform_sampling", "deskew", "transform_cloud", "frontend", "wire", "kf_push_assemble", "kf_select", "pose_graph",
        "map_insert_evict_rebase", "map_commit", "icp", "mapping_registration"]
WARM, REPS = 2, 7


def child():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch  # noqa: F401
    import one_context_ops as oc
    ctx = oc.Ctx()
    res = {}
    for name in ROWS:
        op = oc.OPS[name]
        op.make("large")
        for form in op.forms:
            t = []
            for i in range(WARM + REPS):
                t0 = time.perf_counter()
                op.run(ctx, "large", form)
                ctx.chk(ctx.L.rgc_synchronize(ctx.h))
                t.append(time.perf_counter() - t0)
            res["%s[%s]" % (name, form)] = round(1e6 * statistics.median(t[WARM:]), 2)
    ctx.close()
    print("RESULT " + json.dumps(res))


def main():
    rounds, out = int(sys.argv[1]), os.path.abspath(sys.argv[2])
    libs = {"parent": os.path.abspath(sys.argv[3]), "new": os.path.abspath(sys.argv[4]) if len(sys.argv) > 4 else os.path.join(ROOT, "rgc-slam_amd", "librgc_hip.so")}
    runs, order = {"parent": [], "new": []}, []
    os.makedirs(os.path.dirname(out), exist_ok=True)
    for i in range(rounds):
        for arm in (("parent", "new") if i % 2 == 0 else ("new", "parent")):
            t0 = time.time()
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=dict(os.environ, RGC_HIP_LIB=libs[arm]), capture_output=True, text=True, timeout=300)
            line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                print(arm, "exit", r.returncode, r.stdout[-500:], r.stderr[-2000:], flush=True)
                sys.exit(1)
            runs[arm].append(json.loads(line[-1][7:]))
            order.append(arm)
            print(i, arm, "%.1f s" % (time.time() - t0), flush=True)
            json.dump({"what": __doc__, "unit": "us per row, median of %d after %d" % (REPS, WARM), "order": " ".join(order), "runs": runs}, open(out, "w"), indent=1)


if __name__ == "__main__":
    child() if "--child" in sys.argv else main()
