"""Host-side mirror of the NDT registration (P2D / D2D) on a Gaussian voxel map: fast_gicp::NDTCuda (include/fast_gicp/ndt/ndt_cuda.hpp:27-60,
impl/ndt_cuda_impl.hpp:10-90) behind the rgc_ndt_* entry points of include/rgc_hip.h, with the reference's method names.

    ndt = NDTRegistration(device=0)                 # or NDTRegistration(owner=store_owner): in the context a KeyframeStore assembles in
    ndt.setResolution(1.0); ndt.setDistanceMode(NDT_D2D); ndt.setNeighborSearchMethod(NDT_DIRECT7)
    ndt.setInputTarget(store.assemble(ids, kinds, leaf=0.4, device=True)); ndt.setInputSource(keyframe_cloud)
    T = ndt.align(guess); ok = ndt.hasConverged()

Clouds are numpy arrays (n, >=3) float32 or keyframes.DeviceCloud.  Nothing is computed on the CPU; without librgc_hip.so / an MI355X this raises."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import NDT_P2D, NDT_D2D, NDT_DIRECT27, NDT_DIRECT7, NDT_DIRECT1, NDT_DIRECT_RADIUS, RgcError  # noqa: F401  (re-exported)
from ._lsq import lsq_seam

_dp, _fp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int)


@lsq_seam("linearize", "compute_error")
class NDTRegistration:
    _family = "rgc_ndt"

    def __init__(self, device: int = 0, owner=None, params: "_lib.Params | None" = None):
        self._L = _lib.load()
        self._own = owner is None
        if owner is None:
            h = C.c_void_p()
            rc = self._L.rgc_create(device, C.byref(params) if params is not None else None, C.byref(h))
            if rc:
                raise RgcError(rc, self._L.rgc_status_string(rc).decode())
            self._h = h
        else:
            self._h, self._owner = owner._h, owner
        self._p = _lib.NdtParams()
        self._L.rgc_default_ndt_params(C.byref(self._p))
        self._chk(self._L.rgc_ndt_set_params(self._h, C.byref(self._p)))
        self._T = np.eye(4, dtype=np.float32)
        self._H = np.eye(6)
        self._iterations = 0
        self._converged = self._lm_failed = False

    def close(self):
        if self._own and getattr(self, "_h", None):
            self._L.rgc_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise RgcError(rc, self._L.rgc_last_error(self._h).decode() or self._L.rgc_status_string(rc).decode())

    def _apply(self, **kw):
        p = _lib.NdtParams(self._p.resolution, self._p.distance_mode, self._p.neighbor_method, self._p.neighbor_radius)
        for k, v in kw.items():
            setattr(p, k, v)
        self._chk(self._L.rgc_ndt_set_params(self._h, C.byref(p)))
        self._p = p

    # ---- the reference's setters (ndt_cuda_impl.hpp:19-32) ----
    def setDistanceMode(self, mode): self._apply(distance_mode=int(mode))
    def setResolution(self, resolution): self._apply(resolution=float(resolution))

    def setNeighborSearchMethod(self, method, radius=-1.0):
        if int(method) == NDT_DIRECT_RADIUS:
            self._apply(neighbor_method=int(method), neighbor_radius=float(radius))
        else:
            self._apply(neighbor_method=int(method))

    def getParams(self) -> dict:
        p = _lib.NdtParams()
        self._chk(self._L.rgc_ndt_get_params(self._h, C.byref(p)))
        return dict(resolution=p.resolution, distance_mode=p.distance_mode, neighbor_method=p.neighbor_method, neighbor_radius=p.neighbor_radius)

    def _set(self, host, dev, cloud):
        if hasattr(cloud, "ptr"):                       # keyframes.DeviceCloud
            if cloud._h.value != self._h.value:
                cloud.synchronize()                     # assembled on another context's stream
            self._chk(dev(self._h, cloud.ptr, len(cloud), cloud.stride_bytes))
            return
        a = np.ascontiguousarray(cloud, dtype=np.float32)
        if a.ndim != 2 or a.shape[1] < 3:
            raise RgcError(_lib.ERR_INVALID, "a cloud is (n, >=3) float32: x, y, z first")
        self._chk(host(self._h, a.ctypes.data, a.shape[0], a.strides[0]))

    def setInputTarget(self, cloud): self._set(self._L.rgc_ndt_set_target, self._L.rgc_ndt_set_target_device, cloud)
    def setInputSource(self, cloud): self._set(self._L.rgc_ndt_set_source, self._L.rgc_ndt_set_source_device, cloud)
    def clearSource(self): self._chk(self._L.rgc_ndt_clear_source(self._h))
    def clearTarget(self): self._chk(self._L.rgc_ndt_clear_target(self._h))
    def swapSourceAndTarget(self): self._chk(self._L.rgc_ndt_swap_source_and_target(self._h))

    # ---- LsqRegistration's seam (ndt_cuda_impl.hpp:81-90): linearize and compute_error are _lsq.py's over rgc_ndt_* ----
    def num_correspondences(self) -> int:
        n = C.c_int(0)
        self._chk(self._L.rgc_ndt_num_correspondences(self._h, C.byref(n)))
        return n.value

    def align(self, guess=None):
        g = np.ascontiguousarray(np.eye(4) if guess is None else guess, dtype=np.float32).reshape(16)
        T, H = np.zeros(16, np.float32), np.zeros(36)
        it, cv, lf = C.c_int(0), C.c_int(0), C.c_int(0)
        self._chk(self._L.rgc_ndt_align(self._h, g.ctypes.data_as(_fp), T.ctypes.data_as(_fp), H.ctypes.data_as(_dp), C.byref(it), C.byref(cv), C.byref(lf)))
        self._T, self._H = T.reshape(4, 4), H.reshape(6, 6)
        self._iterations, self._converged, self._lm_failed = it.value, bool(cv.value), bool(lf.value)
        return self._T

    def getFinalTransformation(self): return self._T
    def getFinalHessian(self): return self._H
    def hasConverged(self): return self._converged
    def lmFailed(self): return self._lm_failed
    def iterations(self): return self._iterations

    def voxels(self, which=0, raw=False) -> dict:
        """the voxel map of the target (0) or the source (1): coords (V, 3) int32, n (V,), mean (V, 3), cov (V, 3, 3) after MIN_EIG
        (and cov_raw, before it, when raw)"""
        cnt = C.c_int(0)
        self._chk(self._L.rgc_ndt_get_voxels(self._h, which, 0, None, None, None, None, C.byref(cnt)))
        V = cnt.value
        co, n, m, cv = np.zeros((V, 3), np.int32), np.zeros(V, np.int32), np.zeros((V, 3)), np.zeros((V, 3, 3))
        self._chk(self._L.rgc_ndt_get_voxels(self._h, which, V, co.ctypes.data_as(_ip), n.ctypes.data_as(_ip), m.ctypes.data_as(_dp), cv.ctypes.data_as(_dp), C.byref(cnt)))
        out = dict(coords=co, n=n, mean=m, cov=cv)
        if raw:
            cr = np.zeros((V, 3, 3))
            self._chk(self._L.rgc_ndt_get_raw_covariances(self._h, which, V, cr.ctypes.data_as(_dp), C.byref(cnt)))
            out["cov_raw"] = cr
        return out
