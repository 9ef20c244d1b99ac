"""The touched rows of tests/one_context_ops.py at both sizes, host and device form, one after the other on ONE context: parent library twice, new library once
(each in a child process, loaded through RGC_HIP_LIB); every output, info struct and what each row leaves on the context compared byte for byte.
    python scripts/same_bytes_rows.py OUT_DIR PARENT_LIB [NEW_LIB]"""
import os
import pickle
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = ["voxelgrid", "voxelgrid_in_halves", "uniform_sampling", "deskew", "transform_cloud", "frontend", "wire", "kf_push_assemble", "kf_select", "pose_graph",
        "map_insert_evict_rebase", "map_commit", "icp", "mapping_registration", "vgicp_reframed_target"]


def flat(v, path, out):
    import one_context_ops as oc
    if isinstance(v, dict):
        for k in sorted(v, key=str):
            flat(v[k], path + "/" + str(k), out)
    elif isinstance(v, (list, tuple)):
        for i, x in enumerate(v):
            flat(x, path + "[%d]" % i, out)
    else:
        b = oc._b(v)
        out[path] = b if b[0] != "o" else ("o", repr(v))


def child(out_path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch  # noqa: F401
    import one_context_ops as oc
    ctx = oc.Ctx()
    res, rows = {}, 0
    for size in oc.SIZES:
        for name in ROWS:
            op = oc.OPS[name]
            for form in op.forms:
                key = "%s[%s,%s]" % (name, size, form)
                flat(op.run(ctx, size, form), key + "/out", res)
                flat(op.kept(ctx), key + "/kept", res)
                rows += 1
    ctx.close()
    with open(out_path, "wb") as f:
        pickle.dump((rows, res), f)
    print("child ok", rows, "rows", len(res), "values")


def nbytes(b):
    return len(b[2]) if len(b) == 3 else 8


def main():
    out = os.path.abspath(sys.argv[1])
    os.makedirs(out, exist_ok=True)
    parent, new = os.path.abspath(sys.argv[2]), os.path.abspath(sys.argv[3]) if len(sys.argv) > 3 else os.path.join(ROOT, "rgc-slam_amd", "librgc_hip.so")
    got = []
    for tag, lib in (("parent_a", parent), ("parent_b", parent), ("new", new)):
        p = os.path.join(out, "same_bytes_%s.pkl" % tag)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", p], env=dict(os.environ, RGC_HIP_LIB=lib), capture_output=True, text=True, timeout=400)
        print(tag, r.returncode, r.stdout[-300:].strip(), r.stderr[-1500:].strip(), flush=True)
        if r.returncode != 0:
            sys.exit(r.returncode if r.returncode > 0 else 1)
        got.append(pickle.load(open(p, "rb")))
    (ra, a), (rb, b), (rn, n) = got
    total = sum(nbytes(v) for v in a.values())
    lines = ["rows %d / %d / %d, values %d, bytes compared %d" % (ra, rb, rn, len(a), total)]
    for tag, x in (("parent against parent", b), ("new against parent", n)):
        bad = sorted(set(a) ^ set(x)) + [k for k in a if k in x and a[k] != x[k]]
        lines.append("%s: %d values differ %s" % (tag, len(bad), bad[:10]))
    print("\n".join(lines))
    open(os.path.join(out, "same_bytes.txt"), "w").write("\n".join(lines) + "\n")
    for tag in ("parent_a", "parent_b", "new"):
        os.remove(os.path.join(out, "same_bytes_%s.pkl" % tag))


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        main()
