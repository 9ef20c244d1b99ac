"""Host-side mirror of the outlier filters: pcl::StatisticalOutlierRemoval and pcl::RadiusOutlierRemoval with PCL's member names, behind the
rgc_outlier_* entry points of include/rgc_hip.h (which state the key, the mean distance, the statistics, the decision and the refusals).

    sor = StatisticalOutlierRemoval(device=0)          # or (owner=other): in the context of another object of this package
    sor.setInputCloud(points)                          # (n, >=3) float32, a keyframes.DeviceCloud, or a tensor on the context's GPU
    sor.setMeanK(20); sor.setStddevMulThresh(1.0)
    kept = sor.filter()                                # (m, 4) float32 records x, y, z, c in input order
    sor.getIndices(); sor.getRemovedIndices()          # (m,) / (n - m,) int32, ascending
    sor.getMeanDistances(); sor.info()                 # (n,) float32 of the last filter(); rgc_outlier_info as a dict

    ror = RadiusOutlierRemoval(); ror.setRadiusSearch(0.5); ror.setMinNeighborsInRadius(5); ...   # getCounts() after filter(with_counts=True)

A device cloud is filtered where it lies; its results are computed into device memory and downloaded.  Results are numpy arrays.  Nothing is computed on
the CPU; without librgc_hip.so / an MI355X this raises."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import RgcError, OUTLIER_MAX_MEAN_K  # noqa: F401  (re-exported)
from .search import KdTree


class _OutlierFilter(KdTree):
    """the context, the cloud forms and the device staging are search.KdTree's; the index of that class is not used"""

    def __init__(self, device: int = 0, owner=None):
        super().__init__(device, owner)
        self._cloud = None
        self._negative = False
        self._idx = self._removed = self._val = None

    def setInputCloud(self, points):
        self._cloud = points
        self._idx = self._removed = self._val = None

    def setNegative(self, negative: bool):
        self._negative = bool(negative)

    def getNegative(self) -> bool:
        return self._negative

    def setCell(self, cell: float):
        """the grid's cell size, for tests and tuning (0 = automatic); no output depends on it (rgc_outlier_set_cell)"""
        self._chk(self._L.rgc_outlier_set_cell(self._h, float(cell)))

    def getIndices(self):
        self._need()
        return self._idx

    def getRemovedIndices(self):
        self._need()
        if self._removed is None:
            keep = np.zeros(self._n, bool)
            keep[self._idx] = True
            self._removed = np.flatnonzero(~keep).astype(np.int32)
        return self._removed

    def info(self) -> dict:
        s = _lib.OutlierInfo()
        self._chk(self._L.rgc_outlier_get_info(self._h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in _lib.OutlierInfo._fields_}

    def _need(self):
        if self._idx is None:
            raise RgcError(_lib.ERR_INVALID, "filter() has not run on this cloud")

    def _run(self, call, val_dtype, want_val):
        """call(p, n, stride, on_device, out, idx, val, n_out) -> rc; returns the records"""
        if self._cloud is None:
            raise RgcError(_lib.ERR_NO_INPUT, "no input cloud (setInputCloud)")
        p, n, stride, dev, _keep = self._points(self._cloud)
        out, idx = np.empty((n, 4), np.float32), np.empty(n, np.int32)
        val = np.empty(n, val_dtype) if want_val else None
        kept = C.c_int(0)
        if not dev:
            self._chk(call(p, n, stride, 0, out.ctypes.data, idx.ctypes.data, val.ctypes.data if want_val else None, C.byref(kept)))
        else:
            d_out, d_idx, d_val = self._dev(out.nbytes), self._dev(idx.nbytes), self._dev(4 * n) if want_val else None
            try:
                self._chk(call(p, n, stride, 1, d_out, d_idx, d_val, C.byref(kept)))
                self._down(out[:kept.value], d_out)
                self._down(idx[:kept.value], d_idx)
                if want_val:
                    self._down(val, d_val)
            finally:
                for d in (d_out, d_idx, d_val):
                    if d is not None:
                        self._L.rgc_device_free(self._h, d)
        self._n, self._idx, self._removed, self._val = n, idx[:kept.value].copy(), None, val
        return out[:kept.value].copy()


class StatisticalOutlierRemoval(_OutlierFilter):
    def __init__(self, device: int = 0, owner=None):
        super().__init__(device, owner)
        self._mean_k, self._std_mul = 1, 0.0    # PCL's defaults

    def setMeanK(self, mean_k: int):
        if not 1 <= int(mean_k) <= OUTLIER_MAX_MEAN_K:
            raise RgcError(_lib.ERR_INVALID, f"mean_k in 1..{OUTLIER_MAX_MEAN_K}")
        self._mean_k = int(mean_k)

    def getMeanK(self) -> int:
        return self._mean_k

    def setStddevMulThresh(self, std_mul: float):
        if not np.isfinite(std_mul):
            raise RgcError(_lib.ERR_INVALID, "std_mul must be finite")
        self._std_mul = float(std_mul)

    def getStddevMulThresh(self) -> float:
        return self._std_mul

    def filter(self, with_mean_distances: bool = True):
        """the kept points, (m, 4) float32 in input order"""
        return self._run(lambda p, n, st, dev, out, idx, val, kept: self._L.rgc_outlier_statistical(
            self._h, p, n, st, dev, self._mean_k, self._std_mul, 1 if self._negative else 0, out, idx, val, kept), np.float32, with_mean_distances)

    def getMeanDistances(self):
        """(n,) float32: every point's mean distance to its mean_k nearest neighbours, of the last filter()"""
        self._need()
        return self._val


class RadiusOutlierRemoval(_OutlierFilter):
    def __init__(self, device: int = 0, owner=None):
        super().__init__(device, owner)
        self._radius, self._min_nb = 0.0, 1      # PCL's defaults (a radius must be set before filter())

    def setRadiusSearch(self, radius: float):
        fits = np.isfinite(radius) and float(radius) * float(radius) <= float(np.finfo(np.float32).max)    # float32(r r) is finite
        if not (fits and radius > 0):
            raise RgcError(_lib.ERR_INVALID, "the radius must be finite and > 0, float32(r r) finite")
        self._radius = float(radius)

    def getRadiusSearch(self) -> float:
        return self._radius

    def setMinNeighborsInRadius(self, min_neighbors: int):
        if int(min_neighbors) < 0:
            raise RgcError(_lib.ERR_INVALID, "min_neighbors >= 0")
        self._min_nb = int(min_neighbors)

    def getMinNeighborsInRadius(self) -> int:
        return self._min_nb

    def filter(self, with_counts: bool = False):
        """the kept points, (m, 4) float32 in input order.  with_counts: every point's exact count (getCounts) -- no walk stops early then"""
        return self._run(lambda p, n, st, dev, out, idx, val, kept: self._L.rgc_outlier_radius(
            self._h, p, n, st, dev, self._radius, self._min_nb, 1 if self._negative else 0, out, idx, val, kept), np.int32, with_counts)

    def getCounts(self):
        """(n,) int32: the points within the radius of every point, itself included; None unless the last filter() ran with_counts"""
        self._need()
        return self._val
