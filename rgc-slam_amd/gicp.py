"""Host-side mirror of FastGICP: GICP on an exact nearest neighbour per source point, under the kNN covariances of both clouds --
fast_gicp::FastGICP (include/fast_gicp/gicp/fast_gicp.hpp:25-87, impl/fast_gicp_impl.hpp:103-237) behind the rgc_gicp_* entry points of
include/rgc_hip.h, with the reference's method names.

    gicp = FastGICP(device=0)
    gicp.setCorrespondenceRandomness(20); gicp.setMaxCorrespondenceDistance(1.0)
    gicp.setInputTarget(map_cloud); gicp.setInputSource(scan)
    gicp.align(guess, want_output=False); T = gicp.getFinalTransformation(); ok = gicp.hasConverged()

In the reference FastVGICP derives from FastGICP and inherits its clouds and covariances; here the GICP calls run on the clouds of a
registration.FastVGICP context, so this class derives from that mirror: every way it has of handing a cloud over (host arrays, device
pointers, a re-framed, lazy or borrowed target, caller-set covariances, either covariance route) serves GICP too, and linearize /
compute_error / align / num_correspondences are the GICP ones.  Nothing is computed on the CPU; without librgc_hip.so / an MI355X
constructing one raises."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import RgcError  # noqa: F401  (re-exported)
from .registration import FastVGICP

_dp, _fp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int)


class FastGICP(FastVGICP):
    def setMaxCorrespondenceDistance(self, d):       # fast_gicp_impl.hpp:136: a pair is kept iff its squared distance < d * d
        self._chk(self._L.rgc_gicp_set_max_correspondence_distance(self._h, float(d)))
        self._max_corr_dist = float(d)

    def getMaxCorrespondenceDistance(self) -> float:
        d = C.c_double(0.0)
        self._chk(self._L.rgc_gicp_get_max_correspondence_distance(self._h, C.byref(d)))
        return d.value

    # ---- LsqRegistration's seam (fast_gicp_impl.hpp:155-237) ----
    def linearize(self, T, want_H=True):
        """returns (cost, H, b) -- H and b None unless want_H"""
        T = np.ascontiguousarray(T, dtype=np.float64).reshape(16)
        H, b, cost = np.zeros(36), np.zeros(6), C.c_double(0.0)
        self._chk(self._L.rgc_gicp_linearize(self._h, T.ctypes.data_as(_dp), H.ctypes.data_as(_dp) if want_H else None,
                                             b.ctypes.data_as(_dp) if want_H else None, C.byref(cost)))
        return (cost.value, H.reshape(6, 6), b) if want_H else (cost.value, None, None)

    def compute_error(self, T) -> float:
        T = np.ascontiguousarray(T, dtype=np.float64).reshape(16)
        cost = C.c_double(0.0)
        self._chk(self._L.rgc_gicp_compute_error(self._h, T.ctypes.data_as(_dp), C.byref(cost)))
        return cost.value

    @property
    def num_correspondences(self) -> int:
        n = C.c_int(0)
        self._chk(self._L.rgc_gicp_num_correspondences(self._h, C.byref(n)))
        return n.value

    def correspondences(self):
        """(idx, sq_dist) of the last linearize, in the source's order: idx int32, -1 where rejected; sq_dist float32, the key even there"""
        idx, sq = np.empty(self._n_src, np.int32), np.empty(self._n_src, np.float32)
        self._chk(self._L.rgc_gicp_get_correspondences(self._h, idx.ctypes.data_as(_ip), sq.ctypes.data_as(_fp)))
        return idx, sq

    def align(self, guess=None, want_output=True, want_fitness=False):
        """pcl::Registration::align(output, guess): the transformed source cloud (n, 3) float32, or None if want_output=False"""
        g = np.ascontiguousarray(np.eye(4) if guess is None else guess, dtype=np.float32).reshape(16)
        fin, H = np.empty(16, np.float32), np.empty(36)
        fit = C.c_double(0.0)
        it, cv, lf = C.c_int(0), C.c_int(0), C.c_int(0)
        self._chk(self._L.rgc_gicp_align(self._h, g.ctypes.data_as(_fp), fin.ctypes.data_as(_fp), H.ctypes.data_as(_dp),
                                         C.byref(fit) if want_fitness else None, C.byref(it), C.byref(cv), C.byref(lf)))
        self._final, self._H = fin.reshape(4, 4), H.reshape(6, 6)
        self._iterations, self._converged, self._lm_failed = it.value, bool(cv.value), bool(lf.value)
        self._fitness = fit.value if want_fitness else None
        if not want_output:
            return None
        out = np.empty((self._n_src, 3), np.float32)
        self._chk(self._L.rgc_get_aligned(self._h, fin.ctypes.data_as(_fp), out.ctypes.data_as(_fp), 12))
        return out
