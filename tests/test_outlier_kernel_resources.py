"""Static resources of the outlier filters' kernels (rgc-slam_amd/csrc/rgc_filters.hip), read from the built library's code objects
(scripts/kernel_resources.py, no GPU), after tests/test_search_kernel_resources.py: the set of kernels is the documented one, the mean-distance kernel is
built at its five list tiers (4, 8, 16, 32 and 64 entries) and the count kernel with and without the early exit, and every instantiation has no vector
or scalar spill, no private segment and no accumulator registers -- the per-lane key lists really are registers, the 64-entry tier included.  The vector
register counts and the waves per SIMD are printed, not capped: nobody has tuned the occupancy yet."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_filter_kernel_has_no_spill_no_scratch_and_no_agprs():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    lib = os.path.join(ROOT, "rgc-slam_amd", "librgc_hip.so")
    assert os.path.exists(lib), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    src = open(os.path.join(ROOT, "rgc-slam_amd", "csrc", "rgc_filters.hip")).read()
    defined = set(re.findall(r"__global__\s+void\s+(?:__launch_bounds__\([^)]*\)\s*)?(k_\w+)\s*\(", src))
    assert defined == {"k_sor_meandist", "k_sor_stats", "k_sor_fold", "k_ror_count", "k_outlier_flag", "k_outlier_emit"}, defined
    ks = {k["demangled"]: k for k in m.kernels_of(lib)}
    built = {n: k for n, k in ks.items() if n.split("<")[0].split("(")[0].split("::")[-1] in defined}
    names = sorted(built)
    # five list tiers of the mean-distance kernel, two instantiations of the count kernel, one lane-group size
    assert {n.split("<")[0].split("(")[0].split("::")[-1] for n in built} == defined and len(built) == 11, names
    tiers = sorted(int(re.search(r"k_sor_meandist<(\d+)", n).group(1)) for n in names if "k_sor_meandist<" in n)
    assert tiers == [4, 8, 16, 32, 64], tiers
    assert sorted(re.search(r"k_ror_count<\d+, (\w+)>", n).group(1) for n in names if "k_ror_count<" in n) == ["false", "true"]
    for n, k in sorted(built.items()):
        print("%-40s %3d VGPRs, %3d SGPRs, %5d bytes of LDS, %d waves per SIMD" % (n[:40], k["vgpr"], k["sgpr"], k["lds"], m.waves_per_simd(k)))
        assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0 and k["agpr"] == 0, (n, k)
