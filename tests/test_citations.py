"""The reference citations (file:line) in the header, the oracle, the kernels and the documents resolve: the cited file exists in the reference and the
cited lines are inside it (scripts/check_citations.py, against tests/golden/reference_index.json: the reference's file names, line counts and the public
method names of three headers).  What a citation SAYS about its lines stays a reviewer's job; that it points somewhere real need not be."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_citations_resolve():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "check_citations.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    n = int(r.stdout.split()[0])
    assert n >= 600, r.stdout[:300]


def test_the_adaptor_has_every_public_method_of_the_reference_classes():
    """rgc::FastVGICPHip (rgc-slam_amd/cpp/fast_vgicp_hip.hpp) against the public setters / getters / actions of the classes it stands in for
    (fast_gicp::FastVGICP, FastGICP, LsqRegistration: the names read from the reference's headers) and the pcl::Registration calls of the odometer's
    call site (RGC_odometer.cpp:1000-1011): a user of the reference finds every method name."""
    import json
    import re
    mine = set(re.findall(r"\b(set\w+|get\w+|clear\w+|swap\w+|align\w*|hasConverged)\s*\(", open(os.path.join(ROOT, "rgc-slam_amd", "cpp", "fast_vgicp_hip.hpp")).read()))
    wanted = {"setMaximumIterations", "setMaxCorrespondenceDistance", "setTransformationEpsilon", "setEuclideanFitnessEpsilon", "setRANSACIterations", "setInputTarget",
              "setInputSource", "align", "getFitnessScore", "getFinalTransformation", "hasConverged"}
    methods = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_index.json")))["methods"]
    for f in ("fast_vgicp.hpp", "fast_gicp.hpp", "lsq_registration.hpp"):
        assert methods.get(f), f
        wanted |= set(methods[f])
    assert sorted(wanted - mine) == []
    python_mirror = set(re.findall(r"def (\w+)\(", open(os.path.join(ROOT, "rgc-slam_amd", "registration.py")).read()))     # the same names in the Python mirror
    assert sorted(wanted - python_mirror) == []
