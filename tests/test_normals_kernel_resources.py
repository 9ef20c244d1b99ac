"""Static resources of the normal-estimation kernels (rgc-slam_amd/csrc/rgc_normals.hip), read from the built library's code objects
(scripts/kernel_resources.py, no GPU), after tests/test_plane_kernel_resources.py: the set of kernels is the documented one, the k-route kernel is built at
its four list tiers (4, 8, 16 and 32 packed 64-bit entries) and the radius-route kernel once, at one lane-group size each, and every instantiation has no
vector or scalar spill, no private segment and no accumulator registers -- 32 x 64-bit entries per lane plus the fp64 moments really are registers.  The
vector register counts and the waves per SIMD are printed, not capped."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_normal_kernel_has_no_spill_no_scratch_and_no_agprs():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    lib = os.path.join(ROOT, "rgc-slam_amd", "librgc_hip.so")
    assert os.path.exists(lib), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    src = open(os.path.join(ROOT, "rgc-slam_amd", "csrc", "rgc_normals.hip")).read()
    defined = set(re.findall(r"__global__\s+void\s+(?:__launch_bounds__\([^)]*\)\s*)?(k_\w+)\s*\(", src))
    assert defined == {"k_nrm_check", "k_nrm_knn", "k_nrm_radius"}, defined
    ks = {k["demangled"]: k for k in m.kernels_of(lib)}
    built = {n: k for n, k in ks.items() if n.split("<")[0].split("(")[0].split("::")[-1] in defined}
    names = sorted(built)
    assert {n.split("<")[0].split("(")[0].split("::")[-1] for n in built} == defined and len(built) == 6, names
    tiers = sorted(int(re.search(r"k_nrm_knn<(\d+)", n).group(1)) for n in names if "k_nrm_knn<" in n)
    assert tiers == [4, 8, 16, 32], tiers
    assert len({re.search(r"k_nrm_knn<\d+, (\d+)>", n).group(1) for n in names if "k_nrm_knn<" in n}) == 1 and sum("k_nrm_radius<" in n for n in names) == 1
    for n, k in sorted(built.items()):
        print("%-40s %3d VGPRs, %3d SGPRs, %5d bytes of LDS, %d waves per SIMD" % (n[:40], k["vgpr"], k["sgpr"], k["lds"], m.waves_per_simd(k)))
        assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0 and k["agpr"] == 0, (n, k)
