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

from ._lib import GicpMpParams, RgcError  # noqa: F401  (RgcError re-exported)
from ._lsq import lsq_seam
from .registration import FastVGICP

_dp, _fp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int)


@lsq_seam("linearize", "compute_error", "num_correspondences", "align")
class FastGICP(FastVGICP):
    _family = "rgc_gicp"

    def setMaxCorrespondenceDistance(self, d):       # fast_gicp_impl.hpp:136: a pair is kept iff its squared distance < d * d
        self._chk(self._L.rgc_gicp_set_max_correspondence_distance(self._h, float(d)))
        self._max_corr_dist = float(d)

    def getMaxCorrespondenceDistance(self) -> float:
        d = C.c_double(0.0)
        self._chk(self._L.rgc_gicp_get_max_correspondence_distance(self._h, C.byref(d)))
        return d.value

    # (LsqRegistration's seam, fast_gicp_impl.hpp:155-237: linearize / compute_error / num_correspondences / align are _lsq.py's over rgc_gicp_*)

    def correspondences(self):
        """(idx, sq_dist) of the last linearize, in the source's order: idx int32, -1 where rejected; sq_dist float32, the key even there"""
        idx, sq = np.empty(self._n_src, np.int32), np.empty(self._n_src, np.float32)
        self._chk(self._L.rgc_gicp_get_correspondences(self._h, idx.ctypes.data_as(_ip), sq.ctypes.data_as(_fp)))
        return idx, sq


@lsq_seam("linearize", "compute_error", "num_correspondences", "align")
class FastGICPSingleThread(FastGICP):
    """fast_gicp::FastGICPSingleThread (include/fast_gicp/gicp/fast_gicp_st.hpp:20-65, impl/fast_gicp_st_impl.hpp:19-125) behind rgc_gicpst_*: FastGICP
    whose source points keep an anchor and are searched again only when the triangle inequality cannot prove their nearest neighbour unchanged; a point
    that is not searched keeps its pair, its keys and its Mahalanobis matrix.  Derives from FastGICP as the reference class does: the clouds, the
    covariances and setMaxCorrespondenceDistance are FastGICP's; linearize / compute_error / align / num_correspondences / correspondences are this
    method's.  align() drops the anchors first (:19-22); reset() drops them between linearisations.

        st = FastGICPSingleThread(device=0)
        st.setInputTarget(map_cloud); st.setInputSource(scan)
        st.align(guess, want_output=False); T = st.getFinalTransformation(); searched_last = st.num_searched()"""
    _family = "rgc_gicpst"

    def reset(self):                                  # anchors_.clear() (fast_gicp_st_impl.hpp:20): the next linearize searches every point
        self._chk(self._L.rgc_gicpst_reset(self._h))

    def num_searched(self) -> int:
        """source points the last linearize searched (all of them on the first one after a reset)"""
        n = C.c_int(0)
        self._chk(self._L.rgc_gicpst_num_searched(self._h, C.byref(n)))
        return n.value

    def correspondences(self):
        """(idx, sq_dist, second_sq_dist, searched) after the last linearize, in the source's order: idx int32, -1 where not kept; the fp32 keys to the
        nearest and the second nearest at the point's anchor; searched bool, True where the last linearize searched the point"""
        n = self._n_src
        idx, sq, sq2, was = np.empty(n, np.int32), np.empty(n, np.float32), np.empty(n, np.float32), np.empty(n, np.int32)
        self._chk(self._L.rgc_gicpst_get_correspondences(self._h, idx.ctypes.data_as(_ip), sq.ctypes.data_as(_fp), sq2.ctypes.data_as(_fp), was.ctypes.data_as(_ip)))
        return idx, sq, sq2, was.astype(bool)


@lsq_seam("linearize", "align")
class FastGICPMultiPoints(FastVGICP):
    """fast_gicp::FastGICPMultiPoints (include/fast_gicp/gicp/experimental/fast_gicp_mp.hpp:40-53, fast_gicp_mp_impl.hpp:92-221) behind rgc_gicpmp_*: every
    source point against the distance-weighted merge of every target Gaussian within the search radius, plain Gauss-Newton.  On the clouds of a
    registration.FastVGICP context like FastGICP above; setRotationEpsilon, setTransformationEpsilon and setMaximumIterations set THIS method's limits
    (defaults 1e-5, 1e-5, 64: fast_gicp_mp_impl.hpp:29-31), not the context's LM settings.

        mp = FastGICPMultiPoints(device=0)
        mp.setNeighborSearchRadius(0.5); mp.setInputTarget(map_cloud); mp.setInputSource(scan)
        mp.align(guess, want_output=False); T = mp.getFinalTransformation(); ok = mp.hasConverged()"""
    _family = "rgc_gicpmp"

    def __init__(self, device: int = 0):
        super().__init__(device)
        self._mp = GicpMpParams()
        self._chk(self._L.rgc_gicpmp_get_params(self._h, C.byref(self._mp)))

    def _push_mp(self):
        self._chk(self._L.rgc_gicpmp_set_params(self._h, C.byref(self._mp)))

    def _set_mp(self, name, value):
        old = getattr(self._mp, name)
        setattr(self._mp, name, value)
        try:
            self._push_mp()
        except RgcError:
            setattr(self._mp, name, old)
            raise

    def setNeighborSearchRadius(self, r):             # neighbor_search_radius_ (fast_gicp_mp.hpp:72; the reference has no setter for it)
        self._set_mp("neighbor_search_radius", float(r))

    def getNeighborSearchRadius(self) -> float:
        return self._mp.neighbor_search_radius

    def setRotationEpsilon(self, e):                  # fast_gicp_mp_impl.hpp:42-44
        self._set_mp("rotation_epsilon", float(e))

    def setTransformationEpsilon(self, e):            # pcl::Registration; is_converged, :124
        self._set_mp("transformation_epsilon", float(e))

    def setMaximumIterations(self, n):                # pcl::Registration; :92
        self._set_mp("max_iterations", int(n))

    def setNumThreads(self, n):                       # fast_gicp_mp_impl.hpp:47-55: CPU threads; nothing to set on the GPU
        pass

    def compute_error(self, T):
        raise NotImplementedError("FastGICPMultiPoints has no frozen cost (the reference class has no compute_error)")

    def _counts(self):
        n, m = C.c_int(0), C.c_longlong(0)
        self._chk(self._L.rgc_gicpmp_num_correspondences(self._h, C.byref(n), C.byref(m)))
        return n.value, m.value

    @property
    def num_correspondences(self) -> int:
        """source points with at least one neighbour at the last linearize"""
        return self._counts()[0]

    @property
    def num_pairs(self) -> int:
        """neighbours of all source points at the last linearize"""
        return self._counts()[1]

    @property
    def num_candidates(self) -> int:
        """target points the gather looked at over all source points at the last linearize"""
        m = C.c_longlong(0)
        self._chk(self._L.rgc_gicpmp_num_candidates(self._h, C.byref(m)))
        return m.value

    def merged(self):
        """(count int32 (n,), sum_w (n,), mean (n, 3), cov6 (n, 6: xx xy xz yy yz zz)) of the last linearize, in the source's order"""
        n = self._n_src
        cnt, sw, mean, cov = np.empty(n, np.int32), np.empty(n), np.empty((n, 3)), np.empty((n, 6))
        self._chk(self._L.rgc_gicpmp_get_merged(self._h, cnt.ctypes.data_as(_ip), sw.ctypes.data_as(_dp), mean.ctypes.data_as(_dp), cov.ctypes.data_as(_dp)))
        return cnt, sw, mean, cov

    def neighbors(self, cap=None):
        """(offsets int32 (n + 1,), idx int32, sq_dist float32) of the last linearize: row i is idx[offsets[i]:offsets[i + 1]], original target indices"""
        total = self.num_pairs if cap is None else int(cap)
        off, idx, sq = np.empty(self._n_src + 1, np.int32), np.empty(max(total, 1), np.int32), np.empty(max(total, 1), np.float32)
        nt = C.c_longlong(0)
        self._chk(self._L.rgc_gicpmp_get_neighbors(self._h, off.ctypes.data_as(_ip), idx.ctypes.data_as(_ip), sq.ctypes.data_as(_fp), total, C.byref(nt)))
        return off, idx[:nt.value], sq[:nt.value]
