"""Static resources of the DIRECT_RADIUS kernels (rgc-slam_amd/csrc/rgc_vgicp_radius.hip), read from the built library's code objects
(scripts/kernel_resources.py, metadata only, no GPU): no vector spill, no private segment -- the offset table is read through a pointer, never
held in a per-lane array -- and no accumulator registers, on both covariance routes; the linearisation at the occupancy the 1 / 7 / 27-offset
linearisation has (three waves per SIMD)."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_vgicp_radius_kernel_has_no_spill_no_scratch_and_no_agprs():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    lib = os.path.join(ROOT, "rgc-slam_amd", "librgc_hip.so")
    assert os.path.exists(lib), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    src = open(os.path.join(ROOT, "rgc-slam_amd", "csrc", "rgc_vgicp_radius.hip")).read()
    defined = set(re.findall(r"__global__\s+void\s+(?:__launch_bounds__\([^)]*\)\s*)?(k_\w+)\s*\(", src))
    assert defined == {"k_vgicp_radius_linearize", "k_vr_fold"}, defined
    ks = {k["demangled"]: k for k in m.kernels_of(lib)}
    built = {n: k for n, k in ks.items() if n.split("<")[0] in defined}
    assert set(built) == {"k_vgicp_radius_linearize<true>", "k_vgicp_radius_linearize<false>", "k_vr_fold"}, sorted(built)   # both covariance routes
    for n, k in sorted(built.items()):
        assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0 and k["agpr"] == 0, (n, k)
    for route in ("true", "false"):
        k = built[f"k_vgicp_radius_linearize<{route}>"]
        assert k["vgpr"] <= 168 and k["vgpr"] <= ks["k_linearize"]["vgpr"] + 16, (route, k["vgpr"])   # three waves per SIMD (512 / 3 = 170, granule 8)
        assert k["lds"] <= 4096, (route, k["lds"])                                                   # the block store's rows only
    assert built["k_vr_fold"]["vgpr"] <= 64
