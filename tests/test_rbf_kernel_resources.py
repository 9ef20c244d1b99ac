"""Static resources of the RBF covariance kernel (rgc-slam_amd/csrc/rgc_rbf.hip), read from the built library's code objects (scripts/kernel_resources.py, no
GPU): no vector spill, no private segment and no accumulator registers -- a lane holds ten fp64 sums, its query and a candidate, and the wave's occupancy
is what hides the tile loads of a one-wave workgroup."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_rbf_kernel_has_no_spill_no_scratch_and_no_agprs():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    lib = os.path.join(ROOT, "rgc-slam_amd", "librgc_hip.so")
    assert os.path.exists(lib), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    src = open(os.path.join(ROOT, "rgc-slam_amd", "csrc", "rgc_rbf.hip")).read()
    defined = set(re.findall(r"__global__\s+void\s+(?:__launch_bounds__\([^)]*\)\s*)?(k_\w+)\s*\(", src))
    assert defined == {"k_rbf_cov6"}, defined
    ks = {k["demangled"]: k for k in m.kernels_of(lib)}
    built = {n: k for n, k in ks.items() if n.split("<")[0].split("(")[0].split("::")[-1] in defined}
    assert len(built) == 1, sorted(built)
    for n, k in sorted(built.items()):
        assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0 and k["agpr"] == 0, (n, k)
        assert k["vgpr"] <= 128, (n, k["vgpr"])                                                    # four waves per SIMD at least
