"""Static resources of the FastGICPSingleThread kernels (rgc-slam_amd/csrc/rgc_gicp_st.hip), read from the built library's code objects
(scripts/kernel_resources.py, metadata only, no GPU): every one of them without a vector spill, without a private segment and without accumulator
registers -- the two-nearest search (nn_search2: one more key and one more index than nn_search) keeps the occupancy FastGICP's search has."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_gicp_st_kernel_has_no_spill_no_scratch_and_no_agprs():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    lib = os.path.join(ROOT, "rgc-slam_amd", "librgc_hip.so")
    assert os.path.exists(lib), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    src = open(os.path.join(ROOT, "rgc-slam_amd", "csrc", "rgc_gicp_st.hip")).read()
    defined = set(re.findall(r"__global__\s+void\s+(?:__launch_bounds__\([^)]*\)\s*)?(k_\w+)\s*\(", src))
    assert defined == {"k_gicpst_test", "k_gicpst_search", "k_gicpst_terms", "k_gicpst_export"}, defined
    ks = {k["demangled"]: k for k in m.kernels_of(lib)}
    built = {n: k for n, k in ks.items() if n.split("<")[0] in defined}
    assert {n.split("<")[0] for n in built} == defined and len(built) == 7, sorted(built)          # k_gicpst_terms: four covariance-route pairs
    for n, k in sorted(built.items()):
        assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0 and k["agpr"] == 0, (n, k)
        assert k["vgpr"] <= 128, (n, k["vgpr"])                                                      # four waves per SIMD at least
    search, plain = built["k_gicpst_search"], ks["k_gicp_correspond"]
    assert search["vgpr"] <= 96 and plain["vgpr"] <= 96                                              # both at five waves per SIMD (allocation 88-96)
    assert built["k_gicpst_test"]["vgpr"] <= 64 and built["k_gicpst_export"]["vgpr"] <= 64           # eight waves per SIMD
