"""Host-side mirror of Euclidean cluster extraction: pcl::EuclideanClusterExtraction with PCL's member names, behind the rgc_cluster_* entry points of
include/rgc_hip.h (which state the graph, the clusters, their order and the refusals).

    ec = EuclideanClusterExtraction(device=0)          # or (owner=other): in the context of another object of this package
    ec.setInputCloud(points)                           # (n, >=3) float32, a keyframes.DeviceCloud, or a tensor on the context's GPU
    ec.setClusterTolerance(0.5); ec.setMinClusterSize(10); ec.setMaxClusterSize(25000)
    clusters = ec.extract()                            # a list of int32 index arrays: size descending, then smallest member ascending
    ec.labels()                                        # (n,) int32: the rank of every point's cluster, -1 in none
    ec.offsets(), ec.indices(); ec.info()              # the same clusters in CSR form; rgc_cluster_info as a dict

A device cloud is clustered where it lies; its results are computed into device memory and downloaded.  Results are numpy arrays.  Nothing is computed on
the CPU; without librgc_hip.so / an MI355X this raises."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import RgcError  # noqa: F401  (re-exported)
from .search import KdTree

INT_MAX = 2 ** 31 - 1


def check_tolerance(tolerance):
    """what rgc_cluster_extract accepts: finite, > 0, float32(t t) finite"""
    fits = np.isfinite(tolerance) and float(tolerance) * float(tolerance) <= float(np.finfo(np.float32).max)
    if not (fits and tolerance > 0):
        raise RgcError(_lib.ERR_INVALID, "the tolerance must be finite and > 0, float32(t t) finite")
    return float(tolerance)


class EuclideanClusterExtraction(KdTree):
    """the context, the cloud forms and the device staging are search.KdTree's; the index of that class is not used"""

    def __init__(self, device: int = 0, owner=None):
        super().__init__(device, owner)
        self._cloud = None
        self._tolerance, self._min, self._max = 0.0, 1, INT_MAX      # PCL's defaults (a tolerance must be set before extract())
        self._labels = self._offsets = self._indices = None

    def setInputCloud(self, points):
        self._cloud = points
        self._labels = self._offsets = self._indices = None

    def setClusterTolerance(self, tolerance: float):
        self._tolerance = check_tolerance(tolerance)

    def getClusterTolerance(self) -> float:
        return self._tolerance

    def setMinClusterSize(self, min_size: int):
        if not 1 <= int(min_size) <= INT_MAX:
            raise RgcError(_lib.ERR_INVALID, "min_size in 1..INT_MAX")
        self._min = int(min_size)

    def getMinClusterSize(self) -> int:
        return self._min

    def setMaxClusterSize(self, max_size: int):
        if not 1 <= int(max_size) <= INT_MAX:
            raise RgcError(_lib.ERR_INVALID, "max_size in 1..INT_MAX")
        self._max = int(max_size)

    def getMaxClusterSize(self) -> int:
        return self._max

    def setCell(self, cell: float):
        """the grid's cell size, for tests and tuning (0 = automatic); no output depends on it (rgc_cluster_set_cell)"""
        self._chk(self._L.rgc_cluster_set_cell(self._h, float(cell)))

    def extract(self):
        """the clusters as a list of int32 index arrays (members ascending), size descending then smallest member ascending"""
        if self._cloud is None:
            raise RgcError(_lib.ERR_NO_INPUT, "no input cloud (setInputCloud)")
        if self._max < self._min:
            raise RgcError(_lib.ERR_INVALID, "max_size < min_size")
        p, n, stride, dev, _keep = self._points(self._cloud)
        labels, offsets, indices = np.empty(n, np.int32), np.empty(n + 1, np.int32), np.empty(n, np.int32)
        m = C.c_int(0)
        args = (n, stride, dev, self._tolerance, self._min, self._max)
        if not dev:
            self._chk(self._L.rgc_cluster_extract(self._h, p, *args, labels.ctypes.data, offsets.ctypes.data, indices.ctypes.data, C.byref(m)))
        else:
            d = [self._dev(a.nbytes) for a in (labels, offsets, indices)]
            try:
                self._chk(self._L.rgc_cluster_extract(self._h, p, *args, d[0], d[1], d[2], C.byref(m)))
                self._down(offsets[:m.value + 1], d[1])
                self._down(labels, d[0])
                self._down(indices[:int(offsets[m.value]) if n else 0], d[2])
            finally:
                for x in d:
                    self._L.rgc_device_free(self._h, x)
        self._offsets = offsets[:m.value + 1].copy()
        self._labels, self._indices = labels, indices[:int(self._offsets[-1])].copy()
        return [self._indices[self._offsets[r]:self._offsets[r + 1]] for r in range(m.value)]

    def labels(self):
        """(n,) int32 of the last extract(): the rank of every point's cluster, -1 for a point in no kept cluster"""
        self._need()
        return self._labels

    def offsets(self):
        self._need()
        return self._offsets

    def indices(self):
        self._need()
        return self._indices

    def info(self) -> dict:
        s = _lib.ClusterInfo()
        self._chk(self._L.rgc_cluster_get_info(self._h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in _lib.ClusterInfo._fields_}

    def _need(self):
        if self._labels is None:
            raise RgcError(_lib.ERR_INVALID, "extract() has not run on this cloud")
