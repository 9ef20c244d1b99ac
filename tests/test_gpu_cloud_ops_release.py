"""rgc_destroy gives back every device buffer the six cloud operations allocate (the search index, the outlier filters, cluster extraction, plane
segmentation, normals, FPFH: the records of rgc_ctx.h, released through their bufs() / pinned() / clouds()).

One fresh child process, three cycles of: read the device's free memory, create a context, run every operation once in its HOST form with every optional
output asked for (so that every scratch buffer of the records is allocated) on 300 000-point clouds, destroy the context, synchronise, read free memory
again.  A buffer the library keeps is lost in EVERY cycle; the runtime's one-time pools land in the first cycle only and a neighbour's allocation on a
shared card is not lost every cycle, so the assertion is on the smallest loss of the three: it must not be positive.

That the test can fail was shown once on the MI355X (EXPERIMENTS.md, Round 27): the library as it is loses [171966464, 0, 0] bytes over the three cycles;
a build with one buffer of 300 001 ints left out of OutlierRecord::bufs() loses [174063616, 2097152, 2097152] -- the allocator's 2 MiB granule, every cycle."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import sys
sys.path.insert(0, %r)
import numpy as np
import torch                                     # first: the library's HIP runtime starts beside torch's, not the other way round
free = lambda: (torch.cuda.synchronize(), torch.cuda.mem_get_info()[0])[1]
free()
import rgc_slam_amd.synth as synth
from rgc_slam_amd import features, filters, search, segmentation

N = 300000
_, cloud = synth.make_world_and_map(N, seed=synth.SEED + 27)
_, surface = synth.make_world_and_map(N, seed=synth.SEED + 28)
cloud, surface = np.ascontiguousarray(cloud[:, :3], np.float32), np.ascontiguousarray(surface[:, :3], np.float32)
assert len(cloud) == N and len(surface) == N
rec = np.zeros((N, 4), np.float32)               # whole records with a fourth float: what the filters, clusters and the plane take
rec[:, :3] = cloud
queries = cloud[::8]


def cycle():
    before = free()
    tree = search.KdTree(0)
    tree.setInputCloud(cloud)
    tree.nearestKSearch(queries, 8)
    tree.radiusSearch(queries, 0.5, max_nn=0, sorted=True)
    tree.radiusSearch(queries, 0.5, max_nn=8)
    tree.radiusSearch(cloud[::4096], 8.0, max_nn=0, sorted=True)      # rows beyond the one-pass sort's window: the long sort's second row
    assert tree.info()["rows_sorted_long"] > 0
    sor = filters.StatisticalOutlierRemoval(owner=tree)
    sor.setInputCloud(rec); sor.setMeanK(8); sor.setStddevMulThresh(1.0)
    sor.filter(with_mean_distances=True)
    ror = filters.RadiusOutlierRemoval(owner=tree)
    ror.setInputCloud(rec); ror.setRadiusSearch(0.5); ror.setMinNeighborsInRadius(3)
    ror.filter(with_counts=True)
    ec = segmentation.EuclideanClusterExtraction(owner=tree)
    ec.setInputCloud(rec); ec.setClusterTolerance(0.5); ec.setMinClusterSize(10); ec.setMaxClusterSize(N)
    ec.extract()
    seg = segmentation.SACSegmentation(owner=tree)
    seg.setInputCloud(rec); seg.setDistanceThreshold(0.05); seg.setMaxIterations(20); seg.setOptimizeCoefficients(True)
    seg.setSamples(np.array([[0, N // 2, N - 1], [1, N // 3, N - 2]], np.int32))
    seg.segment(with_counts=True)                 # indices and counts
    seg.filter()                                  # records
    ne = features.NormalEstimation(owner=tree)
    ne.setInputCloud(cloud); ne.setSearchSurface(surface); ne.setKSearch(10)
    ne.compute(with_moments=True)
    ns = features.NormalEstimation(owner=tree)
    ns.setInputCloud(surface); ns.setKSearch(10)
    normals = ns.compute()
    fe = features.FPFHEstimation(owner=tree)
    fe.setInputCloud(cloud); fe.setSearchSurface(surface); fe.setInputNormals(normals); fe.setRadiusSearch(0.6)
    fe.compute(with_spfh=True)
    tree.close()
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
