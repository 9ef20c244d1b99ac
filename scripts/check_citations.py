"""Are the reference citations (file:line) of this repository real?  Every `name.ext:line[-line]` in the given files (default: include/rgc_hip.h, the
oracle's sources, the kernels) whose file name is one of the reference's is resolved and its line range checked against the
file's length.  The reference's files and their lengths come from tests/golden/reference_index.json (paths, line counts and the public method names of
three headers -- no reference text), or from a checkout of the reference given with --reference.  Reports unknown files and ranges past the end; exit
code 1 if any.
    python scripts/check_citations.py [--reference DIR] [files ...]
    python scripts/check_citations.py --write-index DIR      (re-writes the index from a checkout of the reference)"""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INDEX = os.path.join(ROOT, "tests", "golden", "reference_index.json")
DEFAULT = ["include/rgc_hip.h", "oracle/rgc_oracle.c", "oracle/rgc_oracle_aux.c", "oracle/rgc_oracle_map.c", "oracle/rgc_oracle.h", "oracle/py_oracle.py", "oracle/py_frontend.py",
           "oracle/py_fusion.py", "oracle/py_icp.py", "oracle/py_mapreg.py", "oracle/py_odometer.py", "rgc-slam_amd/csrc/rgc_kernels.hip", "rgc-slam_amd/csrc/rgc_api.hip",
           "rgc-slam_amd/csrc/rgc_api_pre.hip", "rgc-slam_amd/csrc/rgc_api_frontend.hip", "rgc-slam_amd/csrc/rgc_api_mapreg.hip", "rgc-slam_amd/csrc/rgc_api_map.hip", "rgc-slam_amd/csrc/rgc_api_wire.hip", "rgc-slam_amd/csrc/rgc_api_icp.hip", "rgc-slam_amd/csrc/rgc_api_keyframes.hip", "rgc-slam_amd/csrc/rgc_api_lsq.hip", "rgc-slam_amd/csrc/rgc_api_ndt.hip", "rgc-slam_amd/csrc/rgc_api_gicp.hip", "rgc-slam_amd/csrc/rgc_ctx.h",
           "rgc-slam_amd/csrc/rgc_frontend.hip", "rgc-slam_amd/csrc/rgc_pre.hip", "rgc-slam_amd/csrc/rgc_host.cpp", "rgc-slam_amd/cpp/odometry_node.hpp",
           "rgc-slam_amd/cpp/fast_vgicp_hip.hpp", "rgc-slam_amd/odometry.py", "rgc-slam_amd/registration.py", "DESIGN.md", "INTEGRATION.md", "SURVEY.md"]
CITE = re.compile(r"([\w/\.]*\b[\w]+\.(?:cpp|hpp|h|cu|cuh|launch|yaml|msg)):(\d+(?:-\d+)?(?:,\s?\d+(?:-\d+)?)*)")


CITED_EXT = (".cpp", ".hpp", ".h", ".cu", ".cuh", ".launch", ".yaml", ".msg")
METHOD = re.compile(r"\b(set\w+|get\w+|clear\w+|swap\w+)\s*\(")
METHOD_HEADERS = ("fast_vgicp.hpp", "fast_gicp.hpp", "lsq_registration.hpp")   # the classes rgc::FastVGICPHip stands in for


def index_of(ref):
    """{"lines": {relative path: line count} of every file a citation can name, "methods": {header: public method names}} of a reference checkout"""
    lines, methods = {}, {}
    for d, _, fs in os.walk(ref):
        for f in sorted(fs):
            p = os.path.join(d, f)
            if f.endswith(CITED_EXT):
                lines[os.path.relpath(p, ref)] = sum(1 for _ in open(p, errors="replace"))
            if f in METHOD_HEADERS and "cuda" not in p:
                methods[f] = sorted(set(METHOD.findall(open(p, errors="replace").read())))
    return {"lines": dict(sorted(lines.items())), "methods": methods}


def load_index(ref=None):
    return index_of(ref) if ref else json.load(open(INDEX))


def reference_files(index):
    by = {}
    for rel in index["lines"]:
        by.setdefault(os.path.basename(rel), []).append(rel)
    return by


def main():
    argv = sys.argv[1:]
    if argv[:1] == ["--write-index"]:
        with open(INDEX, "w") as f:
            json.dump(index_of(argv[1]), f, indent=0)
            f.write("\n")
        return 0
    ref = None
    if argv[:1] == ["--reference"]:
        ref, argv = argv[1], argv[2:]
    index = load_index(ref)
    by = reference_files(index)
    length = index["lines"]
    files = argv or DEFAULT
    total, bad, own = 0, [], 0
    for rel in files:
        p = os.path.join(ROOT, rel)
        if not os.path.exists(p):
            continue
        for ln, line in enumerate(open(p, errors="replace").read().splitlines(), 1):
            for m in CITE.finditer(line):
                name, ranges = m.group(1), m.group(2)
                base = os.path.basename(name)
                if base not in by:
                    if os.path.exists(os.path.join(ROOT, name)) or any(base == os.path.basename(x) for x in DEFAULT) or base.startswith(("rgc_", "test_", "fuzz_")):
                        own += 1            # a citation of this repository's own file
                    else:
                        bad.append((rel, ln, name, ranges, "no such file in the reference"))
                    continue
                cands = [c for c in by[base] if c.endswith(name)] or by[base]
                total += 1
                last = max(int(x) for x in re.findall(r"\d+", ranges))
                ok = False
                for c in cands:
                    ok = ok or last <= length[c]
                if not ok:
                    bad.append((rel, ln, name, ranges, "past the end (%s lines)" % "/".join(str(length[c]) for c in cands)))
    print(f"{total} citations of reference files checked in {len(files)} files ({own} of the repository's own files skipped); {len(bad)} do not resolve")
    for b in bad[:60]:
        print("  %s:%d  %s:%s  -- %s" % b)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
