"""Static resources of the FPFH kernels (rgc-slam_amd/csrc/rgc_fpfh.hip), read from the built library's code objects (scripts/kernel_resources.py, no GPU),
after tests/test_normals_kernel_resources.py: the set of kernels is the documented one, the three walking kernels are built once each (one lane-group size of
the SPFH pass and one of the combine pass ship), and every kernel has no vector or scalar spill, no private segment and no accumulator registers -- the pair
term's fp64 chain with its atan2 and the combine pass' sums really are registers, the 33-counter rows really are LDS.  The register counts, the LDS and the
waves per SIMD are printed, not capped."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_fpfh_kernel_has_no_spill_no_scratch_and_no_agprs():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    lib = os.path.join(ROOT, "rgc-slam_amd", "librgc_hip.so")
    assert os.path.exists(lib), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    src = open(os.path.join(ROOT, "rgc-slam_amd", "csrc", "rgc_fpfh.hip")).read()
    defined = set(re.findall(r"__global__\s+void\s+(?:__launch_bounds__\([^)]*\)\s*)?(k_\w+)\s*\(", src))
    assert defined == {"k_fpfh_check", "k_fpfh_mark", "k_fpfh_list", "k_fpfh_spfh", "k_fpfh_combine"}, defined
    ks = {k["demangled"]: k for k in m.kernels_of(lib)}
    built = {n: k for n, k in ks.items() if n.split("<")[0].split("(")[0].split("::")[-1] in defined}
    names = sorted(built)
    assert {n.split("<")[0].split("(")[0].split("::")[-1] for n in built} == defined and len(built) == 5, names
    for walker in ("k_fpfh_mark<", "k_fpfh_spfh<", "k_fpfh_combine<"):
        assert sum(walker in n for n in names) == 1, (walker, names)
    spfh = next(k for n, k in built.items() if "k_fpfh_spfh<" in n)
    group = int(re.search(r"k_fpfh_spfh<(\d+)>", next(n for n in names if "k_fpfh_spfh<" in n)).group(1))
    assert spfh["lds"] >= (256 // group) * 33 * 4, "a row of 33 counters per surface point of the workgroup"
    for n, k in sorted(built.items()):
        print("%-40s %3d VGPRs, %3d SGPRs, %5d bytes of LDS, %d waves per SIMD" % (n[:40], k["vgpr"], k["sgpr"], k["lds"], m.waves_per_simd(k)))
        assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0 and k["agpr"] == 0, (n, k)
