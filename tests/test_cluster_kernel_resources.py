"""Static resources of the clustering kernels (rgc-slam_amd/csrc/rgc_cluster.hip), read from the built library's code objects
(scripts/kernel_resources.py, no GPU), after tests/test_outlier_kernel_resources.py: the set of kernels is the documented one, the linking kernel is built
at one lane-group size, and every instantiation has no vector or scalar spill, no private segment and no accumulator registers.  The vector register
counts, the LDS and the waves per SIMD are printed, not capped: nobody has tuned the occupancy yet."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {"k_cl_init", "k_cl_link", "k_cl_flatten", "k_cl_census", "k_cl_assign", "k_cl_emit", "k_cl_radix_hist", "k_cl_radix_scatter", "k_cl_rank", "k_cl_labels"}


def test_every_cluster_kernel_has_no_spill_no_scratch_and_no_agprs():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    lib = os.path.join(ROOT, "rgc-slam_amd", "librgc_hip.so")
    assert os.path.exists(lib), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    src = open(os.path.join(ROOT, "rgc-slam_amd", "csrc", "rgc_cluster.hip")).read()
    defined = set(re.findall(r"__global__\s+void\s+(?:__launch_bounds__\([^)]*\)\s*)?(k_\w+)\s*\(", src))
    assert defined == KERNELS, defined
    head = src[:src.index("#include")]
    assert all(k in head for k in KERNELS), "the file's header documents every kernel"
    ks = {k["demangled"]: k for k in m.kernels_of(lib)}
    built = {n: k for n, k in ks.items() if n.split("<")[0].split("(")[0].split("::")[-1] in defined}
    names = sorted(built)
    assert {n.split("<")[0].split("(")[0].split("::")[-1] for n in built} == defined and len(built) == len(KERNELS), names
    assert [re.search(r"k_cl_link<(\d+)", n).group(1) for n in names if "k_cl_link<" in n] == ["4"], "one lane-group size in the product build"
    for n, k in sorted(built.items()):
        print("%-40s %3d VGPRs, %3d SGPRs, %5d bytes of LDS, %d waves per SIMD" % (n[:40], k["vgpr"], k["sgpr"], k["lds"], m.waves_per_simd(k)))
        assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0 and k["agpr"] == 0, (n, k)
