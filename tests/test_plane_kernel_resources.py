"""Static resources of the plane-segmentation kernels (rgc-slam_amd/csrc/rgc_plane.hip), read from the built library's code objects
(scripts/kernel_resources.py, no GPU), after tests/test_cluster_kernel_resources.py: the set of kernels is the documented one, the scoring kernel is built
for one and for four points per thread, the moment kernel for its two passes, and every instantiation has no vector or scalar spill, no private segment
and no accumulator registers.  The register counts, the LDS and the waves per SIMD are printed, not capped: nobody has tuned the occupancy yet."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {"k_pl_models", "k_pl_score", "k_pl_flag", "k_pl_moments", "k_pl_fold_centroid", "k_pl_fold_fit"}


def test_every_plane_kernel_has_no_spill_no_scratch_and_no_agprs():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    lib = os.path.join(ROOT, "rgc-slam_amd", "librgc_hip.so")
    assert os.path.exists(lib), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    src = open(os.path.join(ROOT, "rgc-slam_amd", "csrc", "rgc_plane.hip")).read()
    defined = set(re.findall(r"__global__\s+void\s+(?:__launch_bounds__\([^)]*\)\s*)?(k_\w+)\s*\(", src))
    assert defined == KERNELS, defined
    head = src[:src.index("#include")]
    assert all(k in head for k in KERNELS), "the file's header documents every kernel"
    ks = {k["demangled"]: k for k in m.kernels_of(lib)}
    built = {n: k for n, k in ks.items() if n.split("<")[0].split("(")[0].split("::")[-1] in defined}
    names = sorted(built)
    assert {n.split("<")[0].split("(")[0].split("::")[-1] for n in built} == defined and len(built) == len(KERNELS) + 2, names
    assert sorted(re.search(r"k_pl_score<(\d+)", n).group(1) for n in names if "k_pl_score<" in n) == ["1", "4"], "one and four points per thread"
    assert sorted(re.search(r"k_pl_moments<(\d+)", n).group(1) for n in names if "k_pl_moments<" in n) == ["1", "2"], "the two passes"
    for n, k in sorted(built.items()):
        print("%-40s %3d VGPRs, %3d SGPRs, %5d bytes of LDS, %d waves per SIMD" % (n[:40], k["vgpr"], k["sgpr"], k["lds"], m.waves_per_simd(k)))
        assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0 and k["agpr"] == 0, (n, k)
