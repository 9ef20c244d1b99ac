"""The launch table of a rocprofv3 --kernel-trace csv: one row per (kernel, grid size, workgroup size, LDS bytes) with its launch count, sorted.
With two traces it also says whether the two tables are the same multiset -- what a change of the host code that is meant to leave a frame's
launch sequence alone has to show (run each library over the same driver, e.g. scripts/prof_dependent.py; RGC_HIP_LIB selects the library).
    python scripts/prof_launch_table.py <trace dir A> [<trace dir B>] [--out-a FILE] [--out-b FILE] [--no-params]
--no-params: kernels are named without their parameter lists (a change that retypes a kernel's pointer arguments renames it in the trace)"""
import collections
import csv
import glob
import sys


def without_params(name):
    """k_fold<1>(double const*, int) -> k_fold<1>: cut at the first parenthesis outside the template arguments"""
    depth = 0
    for i, ch in enumerate(name):
        depth += (ch == "<") - (ch == ">")
        if ch == "(" and depth == 0:
            return name[:i]
    return name


def table(trace_dir):
    f = glob.glob(trace_dir + "/**/*kernel_trace.csv", recursive=True)[0]
    rows = list(csv.DictReader(open(f)))
    def dims(r, what):
        return "x".join(r[k] for k in (f"{what}_X", f"{what}_Y", f"{what}_Z") if k in r)
    lds_key = next((k for k in rows[0] if "LDS" in k or "Group_Segment" in k), None)
    t = collections.Counter()
    for r in rows:
        name = r["Kernel_Name"].replace("void ", "").replace("rgck::", "")
        if "--no-params" in sys.argv:
            name = without_params(name)
        t[(name, dims(r, "Grid_Size"), dims(r, "Workgroup_Size"), r[lds_key] if lds_key else "?")] += 1
    return t


def write(t, path):
    lines = [f"{n:6d}  grid {g:>14}  wg {w:>9}  lds {l:>6}  {k}" for (k, g, w, l), n in sorted(t.items())]
    lines.append(f"{sum(t.values())} launches, {len(t)} distinct rows, {len(set(k[0] for k in t))} kernels")
    text = "\n".join(lines) + "\n"
    if path:
        open(path, "w").write(text)
    else:
        sys.stdout.write(text)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = {sys.argv[i]: sys.argv[i + 1] for i in range(1, len(sys.argv) - 1) if sys.argv[i] in ("--out-a", "--out-b")}
    args = [a for a in args if a not in out.values()]
    ta = table(args[0])
    write(ta, out.get("--out-a"))
    if len(args) < 2:
        return
    tb = table(args[1])
    write(tb, out.get("--out-b"))
    same = ta == tb
    print("launch tables (kernel, grid, workgroup, LDS -> count):", "EQUAL" if same else "DIFFERENT")
    for k in sorted(set(ta) | set(tb)):
        if ta.get(k, 0) != tb.get(k, 0):
            print("  ", ta.get(k, 0), "->", tb.get(k, 0), k)
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
