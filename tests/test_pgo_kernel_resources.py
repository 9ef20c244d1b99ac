"""Static resources of the pose-graph kernels (rgc-slam_amd/csrc/rgc_pgo.hip), read from the built library's code objects (scripts/kernel_resources.py, no
GPU): no vector spill, no private segment and no accumulator registers -- the segment kernel keeps the 4x4 fp64 blocks of one elimination step in a
lane's registers, and a spill would put its inner loop into scratch memory."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_pose_graph_kernel_has_no_spill_no_scratch_and_no_agprs():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    lib = os.path.join(ROOT, "rgc-slam_amd", "librgc_hip.so")
    assert os.path.exists(lib), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    src = open(os.path.join(ROOT, "rgc-slam_amd", "csrc", "rgc_pgo.hip")).read()
    defined = set(re.findall(r"__global__\s+void\s+(?:__launch_bounds__\([^)]*\)\s*)?(k_\w+)\s*\(", src))
    assert defined == {"k_pgo_edges", "k_pgo_gather", "k_pgo_fold", "k_pgo_segments", "k_pgo_dense", "k_pgo_backsub", "k_pgo_step"}, defined
    ks = {k["demangled"]: k for k in m.kernels_of(lib)}
    built = {n: k for n, k in ks.items() if n.split("<")[0].split("(")[0].split("::")[-1] in defined}
    assert len(built) == len(defined), sorted(built)
    for n, k in sorted(built.items()):
        assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0 and k["agpr"] == 0, (n, k)
        assert k["vgpr"] <= 256, (n, k["vgpr"])
