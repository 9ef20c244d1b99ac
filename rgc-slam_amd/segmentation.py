"""Host-side mirrors of the segmentation classes: pcl::EuclideanClusterExtraction behind the rgc_cluster_* entry points and pcl::SACSegmentation (RANSAC
plane fit, with the pcl::ExtractIndices step behind it) behind rgc_plane_*, both with PCL's member names; include/rgc_hip.h states the semantics.

    seg = SACSegmentation(device=0)                    # or (owner=other)
    seg.setInputCloud(points); seg.setModelType(SACMODEL_PLANE); seg.setMethodType(SAC_RANSAC)
    seg.setDistanceThreshold(0.2); seg.setMaxIterations(50); seg.setSeed(1)
    inliers, coefficients = seg.segment()              # int32 indices ascending, float64 (a, b, c, d)
    seg.setNegative(True); rest = seg.filter()         # the ground-removed cloud, (m, 4) float32 records in input order

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


SACMODEL_PLANE, SACMODEL_PERPENDICULAR_PLANE = 0, 11   # PCL's enum values (model_types.h) [3P-memory]
SAC_RANSAC = 0                                         # method_types.h; the other methods are not built
_MODEL = {SACMODEL_PLANE: _lib.PLANE_PLANE, SACMODEL_PERPENDICULAR_PLANE: _lib.PLANE_PERPENDICULAR}


class SACSegmentation(KdTree):
    """pcl::SACSegmentation for the two plane models under SAC_RANSAC (rgc_plane_segment); the context, the cloud forms and the device staging are
    search.KdTree's.  The result is a pure function of the cloud, the parameters and the seed (or the samples)."""

    def __init__(self, device: int = 0, owner=None):
        super().__init__(device, owner)
        self._init_params()

    def _init_params(self):
        self._cloud = None
        self._p = _lib.PlaneParams()
        _lib.load().rgc_default_plane_params(C.byref(self._p))
        self._samples, self._negative, self._counts = None, False, None

    def setInputCloud(self, points):
        self._cloud = points

    def setModelType(self, model: int):
        if model not in _MODEL:
            raise RgcError(_lib.ERR_INVALID, "SACMODEL_PLANE or SACMODEL_PERPENDICULAR_PLANE")
        self._p.model_type = _MODEL[model]

    def getModelType(self) -> int:
        return SACMODEL_PERPENDICULAR_PLANE if self._p.model_type == _lib.PLANE_PERPENDICULAR else SACMODEL_PLANE

    def setMethodType(self, method: int):
        if method != SAC_RANSAC:
            raise RgcError(_lib.ERR_INVALID, "only SAC_RANSAC is built")

    def getMethodType(self) -> int:
        return SAC_RANSAC

    def setDistanceThreshold(self, threshold: float):
        t = np.float32(threshold) if np.isfinite(threshold) and abs(threshold) <= float(np.finfo(np.float32).max) else np.float32("nan")
        if not (np.isfinite(t) and t > 0):
            raise RgcError(_lib.ERR_INVALID, "the distance threshold must be finite and > 0 (as a float32 too)")
        self._p.distance_threshold = float(threshold)

    def getDistanceThreshold(self) -> float:
        return self._p.distance_threshold

    def setMaxIterations(self, max_iterations: int):
        if not 1 <= int(max_iterations) <= INT_MAX:
            raise RgcError(_lib.ERR_INVALID, "max_iterations in 1..INT_MAX")
        self._p.max_iterations = int(max_iterations)

    def getMaxIterations(self) -> int:
        return self._p.max_iterations

    def setProbability(self, probability: float):
        if not 0.0 < probability < 1.0:
            raise RgcError(_lib.ERR_INVALID, "probability in (0, 1)")
        self._p.probability = float(probability)

    def getProbability(self) -> float:
        return self._p.probability

    def setOptimizeCoefficients(self, optimize: bool):
        self._p.optimize = 1 if optimize else 0

    def getOptimizeCoefficients(self) -> bool:
        return bool(self._p.optimize)

    def setAxis(self, axis):
        a = np.asarray(axis, np.float64).reshape(-1)
        if a.shape != (3,) or not np.isfinite(a).all() or not np.isfinite(np.sqrt((a * a).sum())) or not (a * a).sum() > 0:
            raise RgcError(_lib.ERR_INVALID, "the axis is three finite numbers, not all zero")
        self._p.axis[:] = [float(v) for v in a]

    def getAxis(self):
        return np.array(list(self._p.axis), np.float64)

    def setEpsAngle(self, eps_angle: float):
        if not 0.0 <= eps_angle <= np.pi / 2:
            raise RgcError(_lib.ERR_INVALID, "eps_angle in [0, pi / 2] radians")
        self._p.eps_angle = float(eps_angle)

    def getEpsAngle(self) -> float:
        return self._p.eps_angle

    def setSeed(self, seed: int):
        """the seed of the generated hypothesis stream (rgc_plane_sample); no PCL counterpart: PCL draws with rand()"""
        self._p.seed = int(seed) & (2 ** 64 - 1)

    def setSamples(self, samples):
        """the hypothesis stream as (m, 3) point indices in place of the generator; None: the generator again"""
        self._samples = None if samples is None else np.ascontiguousarray(samples, np.int32).reshape(-1, 3)

    def setNegative(self, negative: bool):
        """pcl::ExtractIndices::setNegative for filter(): the points that are NOT inliers"""
        self._negative = bool(negative)

    def setBatch(self, batch: int):
        """positions scored per launch, for tests and tuning (0 = automatic); no output depends on it (rgc_plane_set_batch)"""
        self._chk(self._L.rgc_plane_set_batch(self._h, int(batch)))

    def _run(self, negative, want_xyzc, want_index, want_counts=False):
        if self._cloud is None:
            raise RgcError(_lib.ERR_NO_INPUT, "no input cloud (setInputCloud)")
        p, n, stride, dev, _keep = self._points(self._cloud)
        out, idx = np.empty((n if want_xyzc else 0, 4), np.float32), np.empty(n if want_index else 0, np.int32)
        smp, ns = (self._samples.ctypes.data, len(self._samples)) if self._samples is not None else (None, 0)
        length = ns if self._samples is not None else 10 * self._p.max_iterations          # (a count per stream position: asked for explicitly only)
        counts = np.empty(length, np.int32) if want_counts else None
        coeff = np.zeros(4, np.float64)
        m = C.c_int(0)
        head = (self._h, p, n, stride, dev, C.byref(self._p), smp, ns, 1 if negative else 0, coeff.ctypes.data)
        tail = (counts.ctypes.data if want_counts else None, C.byref(m))
        if not dev:
            self._chk(self._L.rgc_plane_segment(*head, out.ctypes.data if want_xyzc else None, idx.ctypes.data if want_index else None, *tail))
        else:
            d_out, d_idx = self._dev(out.nbytes) if want_xyzc else None, self._dev(idx.nbytes) if want_index else None
            try:
                self._chk(self._L.rgc_plane_segment(*head, d_out, d_idx, *tail))
                if want_xyzc:
                    self._down(out[:m.value], d_out)
                if want_index:
                    self._down(idx[:m.value], d_idx)
            finally:
                for x in (d_out, d_idx):
                    if x is not None:
                        self._L.rgc_device_free(self._h, x)
        return out[:m.value].copy(), idx[:m.value].copy(), coeff, counts[:self.info()["positions"]].copy() if want_counts else None

    def segment(self, with_counts: bool = False):
        """(inlier indices (m,) int32 ascending, coefficients (4,) float64: a, b, c, d of a x + b y + c z + d = 0); no model: empty, zeros.
        with_counts: also keep every used position's count for counts() -- one int32 per position of the whole stream is allocated for it"""
        _, idx, coeff, self._counts = self._run(False, False, True, with_counts)
        return idx, coeff

    def filter(self):
        """pcl::ExtractIndices behind segment(): the inliers' (m, 4) float32 records in input order, or with setNegative(True) everything else"""
        out, _, _, _ = self._run(self._negative, True, False)
        return out

    def counts(self):
        """the count of every stream position the last segment(with_counts=True) used, -1 for an invalid one; None without"""
        return self._counts

    def info(self) -> dict:
        s = _lib.PlaneInfo()
        self._chk(self._L.rgc_plane_get_info(self._h, C.byref(s)))
        return {k: (list(getattr(s, k)) if k == "ransac_coeff" else getattr(s, k)) for k, _ in _lib.PlaneInfo._fields_ if k != "reserved"}
