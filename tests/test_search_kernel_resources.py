"""Static resources of the search index's kernels (rgc-slam_amd/csrc/rgc_search.hip), read from the built library's code objects
(scripts/kernel_resources.py, no GPU): the set of kernels is the documented one, and every instantiation has no vector or scalar spill, no private
segment and no accumulator registers -- the per-lane candidate lists of k_search_knn really are registers at every tier (4, 8, 16 and 32 entries).  The
vector register counts and the waves per SIMD are printed, not capped: nobody has tuned the occupancy yet."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_search_kernel_has_no_spill_no_scratch_and_no_agprs():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    lib = os.path.join(ROOT, "rgc-slam_amd", "librgc_hip.so")
    assert os.path.exists(lib), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    src = open(os.path.join(ROOT, "rgc-slam_amd", "csrc", "rgc_search.hip")).read()
    defined = set(re.findall(r"__global__\s+void\s+(?:__launch_bounds__\([^)]*\)\s*)?(k_\w+)\s*\(", src))
    assert defined == {"k_search_knn", "k_search_compact", "k_search_count", "k_search_fill", "k_search_sort_rows", "k_search_unpack"}, defined
    ks = {k["demangled"]: k for k in m.kernels_of(lib)}
    built = {n: k for n, k in ks.items() if n.split("<")[0].split("(")[0].split("::")[-1] in defined}
    names = sorted(built)
    # four list tiers of the top-k kernel, one lane-group size; the small and the window instantiation of the row sort
    assert {n.split("<")[0].split("(")[0].split("::")[-1] for n in built} == defined and len(built) == 10, names
    tiers = sorted(int(re.search(r"k_search_knn<(\d+)", n).group(1)) for n in names if "k_search_knn<" in n)
    assert tiers == [4, 8, 16, 32], tiers
    for n, k in sorted(built.items()):
        print("%-40s %3d VGPRs, %3d SGPRs, %5d bytes of LDS, %d waves per SIMD" % (n[:40], k["vgpr"], k["sgpr"], k["lds"], m.waves_per_simd(k)))
        assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0 and k["agpr"] == 0, (n, k)
    window = [k for n, k in built.items() if "k_search_sort_rows<4096" in n]
    assert len(window) == 1 and window[0]["lds"] == 4096 * 8 and 2 * window[0]["lds"] <= 160 * 1024   # two workgroups and more fit a CU's 160 KiB
