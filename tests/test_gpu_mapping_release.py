"""rgc_destroy gives back every device buffer the mapping side and the stages around the registration allocate (mapping registration, the rolling map, the
keyframe store with its selections, the pose graph, the leaf filter with its staging, ICP, the scan front-end: the records of rgc_ctx.h, released through
their bufs() / pinned() / clouds()).

One fresh child process, three cycles of: read the device's free memory, create the contexts, run every operation once in its HOST form with every optional
output asked for (so that every scratch buffer of the records is allocated) on 300 000-point clouds -- keyframes of 100 000 points per kind, a 64-ring sweep of
300 000 returns --, destroy the contexts, synchronise, read free memory again.  A buffer the library keeps is lost in EVERY cycle; the runtime's one-time pools
land in the first cycle only and a neighbour's allocation on a shared card is not lost every cycle, so the assertion is on the smallest loss of the three: it
must not be positive.  What this cannot see is a buffer below the allocator's granule: tests/test_ctx_records.py reads the lists themselves.

That the test can fail was shown once on the MI355X (EXPERIMENTS.md, Round 28): the library as it is loses [234881024, 0, 0] bytes over the three cycles; a
build with `raw` (the 900 000-point assembly, 14.4 MB grown by half) left out of KeyframeRecord::bufs() loses [257949696, 23068672, 23068672] -- every cycle."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import ctypes as C
import sys
sys.path.insert(0, %r)
import numpy as np
import torch                                     # first: the library's HIP runtime starts beside torch's, not the other way round
free = lambda: (torch.cuda.synchronize(), torch.cuda.mem_get_info()[0])[1]
free()
import rgc_slam_amd.synth as synth
from rgc_slam_amd import frontend, keyframes, local_map, loop_closure, mapping, odometry, pose_graph, registration

N, K = 300000, 100000
world, cloud = synth.make_world_and_map(N, seed=synth.SEED + 29)
_, other = synth.make_world_and_map(N, seed=synth.SEED + 30)
assert len(cloud) == N and len(other) == N
rec, rec2 = np.zeros((N, 4), np.float32), np.zeros((N, 4), np.float32)     # x, y, z and a fourth float: what the map, the store and the filters take
rec[:, :3], rec2[:, :3] = cloud, other
sc = synth.make_scan_n(world, np.eye(4), N, elev_deg=synth.hdl64_elev(), seed=synth.SEED + 31)
sweep = np.ascontiguousarray(np.concatenate([sc["xyz"], sc["intensity"][:, None]], axis=1), np.float32)
assert len(sweep) == N
q0, t0 = np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3)


def cycle():
    before = free()
    # mapping registration: two 300 000-point feature maps, one association, the two-pass solve
    mr = mapping.MapFeatureRegistration(0)
    mr.setInputMaps(rec, rec2)
    mr.associate(rec[::300], q0, t0, "edge")
    mr.optimize(rec[::300], rec2[::100], rec[150::300], rec2[50::100], q0, t0, q0, t0)
    mr.close()
    # the rolling map: three keyframes, an eviction and a re-basing (both stores), the committed target, both downloads
    v = registration.odometer_vgicp(0)
    m = local_map.RollingLocalMap(v)
    m.reset([0.0, 0.0, 0.0])
    for j in range(3):
        m.insert(rec if j != 1 else rec2, q0, [0.5 * j, 0.0, 0.0])
    assert m.evict(max_keyframes=2) == 1
    m.rebase([1.0, 0.0, 0.0])
    assert m.commit(0.3) > 0
    assert len(m.points()) == 2 * N and len(m.target()) > 0
    v.close()
    # the keyframe store, its selections and the pose graph over it
    s = keyframes.KeyframeStore()
    ids = np.array([3, 5, 8], np.int32)
    for j, i in enumerate(ids):
        a = rec if j != 1 else rec2
        s.push(int(i), [0.4 * j, 0.1 * j, 0.0, 0.0, 0.0, 0.02 * j], a[:K], a[K:2 * K], a[2 * K:])
    assert len(s.assemble(ids, (0, 1, 2))) == 9 * K
    assert 0 < len(s.assemble(ids, (0, 1, 2), leaf=0.4)) < 9 * K
    assert len(s.select_surrounding([0.4, 0.1, 0.0], radius=15.0, density=0.3)) > 0
    assert len(s.select_global(0.3)) > 0
    s.detect_loop(min_key_id=0, history_search_num=2)
    g = pose_graph.PoseGraph4DoF(s)
    g.add_loop(8, 3, [-0.8, -0.2, 0.0], -2.0, 0.0, 0.0)
    g.optimize(ids, apply=True)
    s.close()
    # the leaf filter whole and in halves, uniform sampling with indices
    p = odometry.Preprocessor(0)
    L, h = p._L, p._h
    assert len(p.voxelGridFilter(rec, 0.3)) > 0
    d_in, d_out, n_out = C.c_void_p(), C.c_void_p(), C.c_int(0)
    assert L.rgc_device_alloc(h, rec.nbytes, C.byref(d_in)) == 0 and L.rgc_device_alloc(h, rec.nbytes, C.byref(d_out)) == 0
    assert L.rgc_upload(h, d_in, rec.ctypes.data, rec.nbytes) == 0
    assert L.rgc_voxelgrid_begin(h, d_in, N, 16, C.c_float(0.3), d_out) == 0
    assert L.rgc_voxelgrid_end(h, C.byref(n_out)) == 0 and n_out.value > 0
    L.rgc_device_free(h, d_in); L.rgc_device_free(h, d_out)
    pts, idx = p.uniformSampling(rec, 0.5, return_index=True)
    assert len(pts) == len(idx) > 0
    p.close()
    # loop-closure ICP
    icp = loop_closure.IterativeClosestPoint(0)
    icp.setMaximumIterations(5)
    icp.setInputSource(rec[::8] + np.float32([0.05, -0.02, 0.0, 0.0]))
    icp.setInputTarget(rec)
    icp.align()
    icp.close()
    # the front-end on a 64-ring sweep: the ground list and every diagnostic
    fe = frontend.ScanRegistration(64)
    out = fe.laserCloudHandler(sweep, diagnostics=True, cloud=True)
    assert out["n_cloud"] > 0
    fe.close()
    return before - free()


lost = [cycle() for _ in range(3)]
print("device bytes not given back, per cycle:", lost)
assert min(lost) <= 0, lost
print("child ok")
"""


def test_destroy_gives_device_memory_back():
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "child ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
