"""Host-side mirror of surface normal estimation: pcl::NormalEstimation with PCL's member names, behind the rgc_normal_* entry points of
include/rgc_hip.h (which state the neighbourhood, the moments, the normal, the sign rule, the curvature and the refusals).

    ne = NormalEstimation(device=0)                    # or (owner=other): in the context of another object of this package
    ne.setInputCloud(points)                           # (n, >=3) float32, a keyframes.DeviceCloud, or a tensor on the context's GPU
    ne.setSearchSurface(dense)                         # optional: the cloud the neighbours come from (None: the input cloud itself)
    ne.setKSearch(10)                                  # or ne.setRadiusSearch(0.5): exactly one of the two
    ne.setViewPoint(0.0, 0.0, 0.0)
    normals = ne.compute()                             # (n, 4) float32 rows nx, ny, nz, curvature; NaN rows where fewer than three neighbours
    ne.getCovariances(); ne.getCentroids(); ne.getCounts(); ne.info()   # of the last compute(with_moments=True): (n, 6) / (n, 3) float64, (n,) int32

A device cloud is used where it lies; its results are computed into device memory and downloaded.  Results are numpy arrays.  Nothing is computed on
the CPU; without librgc_hip.so / an MI355X this raises.

FPFHEstimation (pcl::FPFHEstimation, the rgc_fpfh_* entry points) is the consumer of those normals; its own docstring shows the calls."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import RgcError, NORMAL_MAX_K  # noqa: F401  (re-exported)
from .search import KdTree


class NormalEstimation(KdTree):
    """the context, the cloud forms and the device staging are search.KdTree's; the index of that class is not used"""

    def __init__(self, device: int = 0, owner=None):
        super().__init__(device, owner)
        self._init_params()

    def _init_params(self):
        self._cloud = self._surface = None
        self._k, self._radius, self._flip = 0, 0.0, True   # PCL's defaults: a caller must choose a route
        self._vp = (0.0, 0.0, 0.0)
        self._cov = self._cen = self._cnt = None
        self._n_valid = None

    def setInputCloud(self, points):
        self._cloud = points
        self._cov = self._cen = self._cnt = self._n_valid = None

    def setSearchSurface(self, points):
        self._surface = points

    def setKSearch(self, k: int):
        """3 .. NORMAL_MAX_K selects the k route (and clears a radius); 0 deselects it"""
        k = int(k)
        if k != 0 and not 3 <= k <= NORMAL_MAX_K:
            raise RgcError(_lib.ERR_INVALID, f"k in 3..{NORMAL_MAX_K} (0: not this route)")
        self._k = k
        if k:
            self._radius = 0.0

    def getKSearch(self) -> int:
        return self._k

    def setRadiusSearch(self, radius: float):
        """> 0 selects the radius route (and clears k); 0 deselects it"""
        radius = float(radius)
        if radius != 0.0:
            with np.errstate(over="ignore"):
                r2 = np.float32(radius * radius) if np.isfinite(radius) else np.float32(np.inf)
            if not (np.isfinite(radius) and radius > 0 and np.isfinite(r2) and r2 > 0):
                raise RgcError(_lib.ERR_INVALID, "the radius must be finite and > 0, float32(r r) finite and > 0")
        self._radius = radius
        if radius:
            self._k = 0

    def getRadiusSearch(self) -> float:
        return self._radius

    def setViewPoint(self, vpx: float, vpy: float, vpz: float):
        with np.errstate(over="ignore"):
            vp = (float(np.float32(vpx)), float(np.float32(vpy)), float(np.float32(vpz)))
        if not all(np.isfinite(v) for v in vp):
            raise RgcError(_lib.ERR_INVALID, "the viewpoint must be finite (as float32 too)")
        self._vp = vp

    def getViewPoint(self):
        return self._vp

    def setFlip(self, flip: bool):
        """True (PCL): flipNormalTowardsViewpoint; False: the component of largest magnitude is made positive"""
        self._flip = bool(flip)

    def setCell(self, cell: float):
        """the grid's cell size, for tests and tuning (0 = automatic) (rgc_normal_set_cell)"""
        self._chk(self._L.rgc_normal_set_cell(self._h, float(cell)))

    def info(self) -> dict:
        s = _lib.NormalInfo()
        self._chk(self._L.rgc_normal_get_info(self._h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in _lib.NormalInfo._fields_}

    def _params(self):
        p = _lib.NormalParams()
        p.k, p.flip, p.radius = self._k, 1 if self._flip else 0, self._radius
        p.viewpoint[:] = self._vp
        return p

    def compute(self, with_moments: bool = False):
        """(n, 4) float32: nx, ny, nz, curvature of every input point; with_moments: the covariances, centroids and counts are kept too"""
        if self._cloud is None:
            raise RgcError(_lib.ERR_NO_INPUT, "no input cloud (setInputCloud)")
        if (self._k != 0) == (self._radius != 0.0):
            raise RgcError(_lib.ERR_INVALID, "exactly one of setKSearch and setRadiusSearch selects the neighbourhood")
        p, n, stride, dev, _keep = self._points(self._cloud)
        sp, ns, sstride, _keep2 = None, 0, 0, None
        if self._surface is not None:
            sp, ns, sstride, sdev, _keep2 = self._points(self._surface)
            if sdev != dev:
                raise RgcError(_lib.ERR_INVALID, "the input cloud and the search surface are both host memory or both device memory")
        prm = self._params()
        out = np.empty((n, 4), np.float32)
        cov = np.empty((n, 6), np.float64) if with_moments else None
        cen = np.empty((n, 3), np.float64) if with_moments else None
        cnt = np.empty(n, np.int32) if with_moments else None
        valid = C.c_int(0)
        ptr = lambda a: a.ctypes.data if a is not None else None
        if not dev:
            self._chk(self._L.rgc_normal_estimate(self._h, p, n, stride, sp, ns, sstride, 0, C.byref(prm), ptr(out), ptr(cov), ptr(cen), ptr(cnt), C.byref(valid)))
        else:
            hosts = (out, cov, cen, cnt)
            devs = [self._dev(a.nbytes) if a is not None else None for a in hosts]
            try:
                self._chk(self._L.rgc_normal_estimate(self._h, p, n, stride, sp, ns, sstride, 1, C.byref(prm), *devs, C.byref(valid)))
                for a, d in zip(hosts, devs):
                    if a is not None:
                        self._down(a, d)
            finally:
                for d in devs:
                    if d is not None:
                        self._L.rgc_device_free(self._h, d)
        self._cov, self._cen, self._cnt, self._n_valid = cov, cen, cnt, valid.value
        return out

    def getCovariances(self):
        """(n, 6) float64 {xx, xy, xz, yy, yz, zz} of the last compute(with_moments=True), else None"""
        return self._cov

    def getCentroids(self):
        return self._cen

    def getCounts(self):
        return self._cnt

    def getValidCount(self):
        """queries with three members or more, of the last compute()"""
        return self._n_valid


class FPFHEstimation(KdTree):
    """pcl::FPFHEstimation with PCL's member names, behind the rgc_fpfh_* entry points of include/rgc_hip.h (which state the rows, the pair term, the
    SPFH counts, the weighting, the normalisation and the refusals).  The context, the cloud forms and the device staging are search.KdTree's.

        fe = FPFHEstimation(device=0)                      # or (owner=other): in the context of another object of this package
        fe.setInputCloud(keypoints)                        # (n, >=3) float32, a keyframes.DeviceCloud, or a tensor on the context's GPU
        fe.setSearchSurface(dense)                         # optional: the cloud the neighbours come from (None: the input cloud itself)
        fe.setInputNormals(normals)                        # (n_surface, >=3) float32 in any of those forms: NormalEstimation.compute()'s rows as they are
        fe.setRadiusSearch(0.5)
        fpfh = fe.compute()                                # (n, 33) float32; NaN rows where a query has no member
        fe.getSPFH(); fe.getCounts(); fe.getValidCount(); fe.info()   # of the last compute(with_spfh=True): ((n_surface, 33) uint32, (n_surface,) int32), (n,) int32"""

    def __init__(self, device: int = 0, owner=None):
        super().__init__(device, owner)
        self._init_params()

    def _init_params(self):
        self._cloud = self._surface = self._normals = None
        self._radius = 0.0                                   # a caller must choose
        self._spfh = self._spfh_cnt = self._cnt = self._n_valid = None

    def setInputCloud(self, points):
        self._cloud = points
        self._spfh = self._spfh_cnt = self._cnt = self._n_valid = None

    def setSearchSurface(self, points):
        self._surface = points

    def setInputNormals(self, normals):
        """one row per SURFACE point (per input point without a search surface): nx, ny, nz first; used as given"""
        self._normals = normals

    def setRadiusSearch(self, radius: float):
        radius = float(radius)
        with np.errstate(over="ignore"):
            r2 = np.float32(radius * radius) if np.isfinite(radius) else np.float32(np.inf)
        if not (np.isfinite(radius) and radius > 0 and np.isfinite(r2) and r2 > 0):
            raise RgcError(_lib.ERR_INVALID, "the radius must be finite and > 0, float32(r r) finite and > 0")
        self._radius = radius

    def getRadiusSearch(self) -> float:
        return self._radius

    def setCell(self, cell: float):
        """the grid's cell size, for tests and tuning (0 = automatic) (rgc_fpfh_set_cell)"""
        self._chk(self._L.rgc_fpfh_set_cell(self._h, float(cell)))

    def info(self) -> dict:
        s = _lib.FpfhInfo()
        self._chk(self._L.rgc_fpfh_get_info(self._h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in _lib.FpfhInfo._fields_ if k != "reserved"}

    def compute(self, with_spfh: bool = False):
        """(n, 33) float32 descriptors of every input point; with_spfh: the first pass' counts and row sizes are kept too (getSPFH)"""
        if self._cloud is None:
            raise RgcError(_lib.ERR_NO_INPUT, "no input cloud (setInputCloud)")
        if self._normals is None:
            raise RgcError(_lib.ERR_NO_INPUT, "no normals (setInputNormals)")
        if self._radius == 0.0:
            raise RgcError(_lib.ERR_INVALID, "no radius (setRadiusSearch)")
        p, n, stride, dev, _keep = self._points(self._cloud)
        sp, ns, sstride, _keep2 = None, 0, 0, None
        if self._surface is not None:
            sp, ns, sstride, sdev, _keep2 = self._points(self._surface)
            if sdev != dev:
                raise RgcError(_lib.ERR_INVALID, "the input cloud, the search surface and the normals are all host memory or all device memory")
        npt, nn, nstride, ndev, _keep3 = self._points(self._normals)
        rows = ns if self._surface is not None else n
        if ndev != dev or nn != rows:
            raise RgcError(_lib.ERR_INVALID, "one normal per surface point, in the memory the clouds are in")
        prm = _lib.FpfhParams()
        prm.radius = self._radius
        out = np.empty((n, _lib.FPFH_BINS), np.float32)
        cnt = np.empty(n, np.int32)
        spfh = np.empty((rows, _lib.FPFH_BINS), np.uint32) if with_spfh else None
        scnt = np.empty(rows, np.int32) if with_spfh else None
        valid = C.c_int(0)
        ptr = lambda a: a.ctypes.data if a is not None else None
        hosts = (out, spfh, scnt, cnt)
        if not dev:
            self._chk(self._L.rgc_fpfh_estimate(self._h, p, n, stride, sp, ns, sstride, npt, nstride, 0, C.byref(prm), *[ptr(a) for a in hosts], C.byref(valid)))
        else:
            devs = [self._dev(a.nbytes) if a is not None else None for a in hosts]
            try:
                self._chk(self._L.rgc_fpfh_estimate(self._h, p, n, stride, sp, ns, sstride, npt, nstride, 1, C.byref(prm), *devs, C.byref(valid)))
                for a, d in zip(hosts, devs):
                    if a is not None:
                        self._down(a, d)
            finally:
                for d in devs:
                    if d is not None:
                        self._L.rgc_device_free(self._h, d)
        self._spfh, self._spfh_cnt, self._cnt, self._n_valid = spfh, scnt, cnt, valid.value
        return out

    def getSPFH(self):
        """((n_surface, 33) uint32 counts, (n_surface,) int32 row sizes, -1 where not computed) of the last compute(with_spfh=True), else (None, None)"""
        return self._spfh, self._spfh_cnt

    def getCounts(self):
        """(n,) int32: the row size of every query, of the last compute()"""
        return self._cnt

    def getValidCount(self):
        """queries with at least one member, of the last compute()"""
        return self._n_valid
