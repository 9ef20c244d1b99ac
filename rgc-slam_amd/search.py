"""Host-side mirror of the search index: pcl::KdTreeFLANN's nearestKSearch / radiusSearch for batches of queries, behind the rgc_search_* entry
points of include/rgc_hip.h (which state the key, the order, the sentinel form of a short row and the refusals).

    tree = KdTree(device=0)                    # or KdTree(owner=store_owner): in the context a KeyframeStore assembles in
    tree.setInputCloud(points)                 # (n, >=3) float32, a keyframes.DeviceCloud, or a tensor on the context's GPU
    idx, sq = tree.nearestKSearch(queries, 5)  # (nq, 5) int32 / float32; -1 / +inf behind min(k, n)
    off, idx, sq = tree.radiusSearch(queries, 1.0, max_nn=0, sorted=True)   # CSR rows: idx[off[i]:off[i + 1]]

Queries are numpy arrays, a DeviceCloud, or any object with ``data_ptr()`` that lies on the context's GPU (a torch ROCm tensor of float32 rows);
device queries are searched where they lie, their rows are computed into device memory and downloaded.  Results are numpy arrays.  Nothing is
computed on the CPU; without librgc_hip.so / an MI355X this raises."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import RgcError, SEARCH_MAX_K  # noqa: F401  (re-exported)


def sort_window() -> int:
    """radius rows up to this many members are sorted in one pass (rgc_search_sort_window)"""
    return int(_lib.load().rgc_search_sort_window())


class KdTree:
    def __init__(self, device: int = 0, owner=None):
        self._L = _lib.load()
        self._own = owner is None
        if owner is None:
            h = C.c_void_p()
            rc = self._L.rgc_create(device, None, C.byref(h))
            if rc:
                raise RgcError(rc, self._L.rgc_status_string(rc).decode())
            self._h = h
        else:
            self._h, self._owner = owner._h, owner

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

    def _points(self, cloud):
        """(pointer, n, stride_bytes, on_device, keep-alive) of a cloud in any accepted form"""
        if hasattr(cloud, "ptr"):                            # keyframes.DeviceCloud
            if cloud._h.value != self._h.value:
                cloud.synchronize()                          # assembled on another context's stream
            return cloud.ptr, len(cloud), cloud.stride_bytes, 1, cloud
        if hasattr(cloud, "data_ptr"):                       # a tensor: float32 rows of >= 3 columns on the GPU
            if not getattr(cloud, "is_cuda", False):
                cloud = cloud.detach().cpu().numpy()
            else:
                if cloud.dim() != 2 or cloud.shape[1] < 3 or cloud.element_size() != 4 or not cloud.is_floating_point() or cloud.stride(1) != 1:
                    raise RgcError(_lib.ERR_INVALID, "a device cloud is (n, >=3) float32 with unit column stride")
                return cloud.data_ptr(), int(cloud.shape[0]), int(cloud.stride(0)) * 4, 1, cloud
        a = np.ascontiguousarray(cloud, dtype=np.float32)
        if a.ndim != 2 or a.shape[1] < 3:
            raise RgcError(_lib.ERR_INVALID, "a cloud is (n, >=3) float32: x, y, z first")
        return a.ctypes.data, a.shape[0], a.strides[0], 0, a

    # ---- pcl::KdTreeFLANN's members ----
    def setInputCloud(self, points, cell: float = 0.0):
        p, n, stride, dev, _keep = self._points(points)
        self._chk(self._L.rgc_search_set_cloud(self._h, p, n, stride, dev, float(cell)))

    def clear(self):
        self._chk(self._L.rgc_search_clear(self._h))

    def info(self) -> dict:
        s = _lib.SearchInfo()
        self._chk(self._L.rgc_search_get_info(self._h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in _lib.SearchInfo._fields_}

    def _dev(self, nbytes):
        d = C.c_void_p()
        self._chk(self._L.rgc_device_alloc(self._h, max(int(nbytes), 16), C.byref(d)))
        return d

    def _down(self, out, d):
        if out.nbytes:
            self._chk(self._L.rgc_download(self._h, out.ctypes.data, d, out.nbytes))

    def nearestKSearch(self, queries, k: int):
        """(idx (nq, k) int32, sq_dist (nq, k) float32): row i = the min(k, n) nearest indexed points of query i, ascending (key, index)"""
        p, nq, stride, dev, _keep = self._points(queries)
        k = int(k)
        idx, sq = np.empty((nq, max(k, 0)), np.int32), np.empty((nq, max(k, 0)), np.float32)
        if not dev:
            self._chk(self._L.rgc_search_knn(self._h, p, nq, stride, 0, k, idx.ctypes.data, sq.ctypes.data))
            return idx, sq
        d_idx, d_sq = self._dev(idx.nbytes), self._dev(sq.nbytes)
        try:
            self._chk(self._L.rgc_search_knn(self._h, p, nq, stride, 1, k, d_idx, d_sq))
            self._down(idx, d_idx)
            self._down(sq, d_sq)
        finally:
            self._L.rgc_device_free(self._h, d_idx)
            self._L.rgc_device_free(self._h, d_sq)
        return idx, sq

    def radiusSearch(self, queries, radius: float, max_nn: int = 0, sorted: bool = True):
        """(offsets (nq + 1,) int32, idx (total,) int32, sq_dist (total,) float32): row i = idx[offsets[i]:offsets[i + 1]], the points with
        key < float32(radius^2); max_nn > 0: the max_nn nearest of them.  Two calls: the first sizes the rows (the cap protocol)."""
        p, nq, stride, dev, _keep = self._points(queries)
        total = C.c_longlong(0)
        args = (self._h, p, nq, stride, dev, float(radius), int(max_nn), 1 if sorted else 0)
        rc = self._L.rgc_search_radius(*args, None, None, None, 0, C.byref(total))
        if rc and not (rc == _lib.ERR_INVALID and total.value > 0):
            self._chk(rc)
        n = int(total.value)
        off, idx, sq = np.zeros(nq + 1, np.int32), np.empty(n, np.int32), np.empty(n, np.float32)
        if not dev:
            self._chk(self._L.rgc_search_radius(*args, off.ctypes.data, idx.ctypes.data, sq.ctypes.data, n, C.byref(total)))
            return off, idx, sq
        d_off, d_idx, d_sq = self._dev(off.nbytes), self._dev(idx.nbytes), self._dev(sq.nbytes)
        try:
            self._chk(self._L.rgc_search_radius(*args, d_off, d_idx, d_sq, n, C.byref(total)))
            self._down(off, d_off)
            self._down(idx, d_idx)
            self._down(sq, d_sq)
        finally:
            for d in (d_off, d_idx, d_sq):
                self._L.rgc_device_free(self._h, d)
        return off, idx, sq
