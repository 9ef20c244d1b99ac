"""Static resources of the FastGICPMultiPoints kernels (rgc-slam_amd/csrc/rgc_gicp_mp.hip), read from the built library's code objects
(scripts/kernel_resources.py, no GPU): every one of them without a vector spill, without a private segment and without accumulator registers -- the fp32
radius gather with its eleven fp64 accumulators and the fp64 term with its thirty are two kernels so that neither has to share its registers with the
other.  The vector register counts are printed, not capped: nobody has tuned the gather's occupancy yet."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_gicp_mp_kernel_has_no_spill_no_scratch_and_no_agprs():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    lib = os.path.join(ROOT, "rgc-slam_amd", "librgc_hip.so")
    assert os.path.exists(lib), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    src = open(os.path.join(ROOT, "rgc-slam_amd", "csrc", "rgc_gicp_mp.hip")).read()
    defined = set(re.findall(r"__global__\s+void\s+(?:__launch_bounds__\([^)]*\)\s*)?(k_\w+)\s*\(", src))
    assert defined == {"k_gicp_mp_merge", "k_gicp_mp_terms", "k_gicp_mp_fold", "k_gicp_mp_export", "k_gicp_mp_fill"}, defined
    ks = {k["demangled"]: k for k in m.kernels_of(lib)}
    built = {n: k for n, k in ks.items() if n.split("<")[0] in defined}
    # the gather: one lane-group size, the target's two covariance routes; the term: the source's two
    assert {n.split("<")[0] for n in built} == defined and len(built) == 7, sorted(built)
    for n, k in sorted(built.items()):
        print("%-32s %3d VGPRs, %3d SGPRs, %5d bytes of LDS, %d waves per SIMD" % (n, k["vgpr"], k["sgpr"], k["lds"], m.waves_per_simd(k)))
        assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0 and k["agpr"] == 0, (n, k)
