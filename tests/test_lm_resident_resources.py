"""Static resources of the resident LM solve (k_lm_solve), read from the built library's code objects (scripts/kernel_resources.py, no GPU):
it runs one workgroup of 256 threads per CU for a whole solve, on the frame's critical path -- no vector spill, no scratch, no accumulator
registers, LDS within a CU's 64 KB, and a register allocation that admits the workgroup it is launched with."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCHED_THREADS = 256   # LIN_T: one virtual block per workgroup


def _table():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    lib = os.path.join(ROOT, "rgc-slam_amd", "librgc_hip.so")
    assert os.path.exists(lib), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    return m, {k["demangled"]: k for k in m.kernels_of(lib)}


def test_k_lm_solve_resources():
    m, ks = _table()
    assert "k_lm_solve" in ks, sorted(n for n in ks if "lm" in n)
    k = ks["k_lm_solve"]
    print(k)
    assert k["vgpr_spill"] == 0 and k["scratch"] == 0 and k["agpr"] == 0, k
    assert k["lds"] <= 64 * 1024, k
    # four SIMDs per CU, 64 lanes per wave: the workgroup's waves must fit the CU at this register allocation
    assert m.waves_per_simd(k) * 4 * 64 >= LAUNCHED_THREADS, k
