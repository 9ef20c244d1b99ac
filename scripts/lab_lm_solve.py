"""Developer aid (library built with RGC_EXTRA_FLAGS=-DRGC_LAB): the period of a try INSIDE the resident solve (k_lm_solve) -- workgroup 0
stamps the 100 MHz wall clock at the top of each of its first 13 tries: per-point work, row store, hand-over, fold, decision.  The headline's
sizes (30 k-point scan, 1 M-point map); RGC_LM_IMPL=chained prints nothing useful (those stamps are k_lm_step's phases: scripts/lab_lm.py)."""
import sys, os, ctypes as C
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import rgc_slam_amd.synth as synth
from rgc_slam_amd import registration, _lib
lib = _lib.load()
lib.rgc_lab_lm_ts.argtypes = [C.c_void_p, C.c_void_p]
world, tgt = synth.make_world_and_map(1000000, seed=synth.SEED)
poses = synth.make_trajectory(4, seed=synth.SEED)
src = synth.make_scan_n(world, poses[1], 30000, seed=synth.SEED + 100)["xyz"]
v = registration.odometer_vgicp(0)
v.setInputTarget(tgt)
ts = np.zeros(16, np.uint64)
lib.rgc_lab_lm_ts(v._h, ts.ctypes.data)
allp = []
for rep in range(8):
    v.setInputSource(src)
    v.align(np.eye(4, dtype=np.float32))
    lib.rgc_lab_lm_ts(v._h, ts.ctypes.data)
    t = [int(x) for x in list(ts[:5]) + list(ts[8:]) if int(x) != 2**64 - 1]   # (slots 5-7 are lm_step_decide's own stamps)
    per = [(b - a) * 10 for a, b in zip(t, t[1:])]
    print("solve", rep, "iterations", v.nr_iterations, "tries stamped", len(t), "ns per try", per, "fallbacks", v.stats()["lm_fallbacks"])
    if rep: allp += per
if allp: print("median ns per try (hand-over included): %d  mean %d" % (int(np.median(allp)), int(np.mean(allp))))
v.close()
