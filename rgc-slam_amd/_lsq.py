"""LsqRegistration's seam (linearize / compute_error / num_correspondences / align) over one family of entry points of include/rgc_hip.h, written once
for the mirrors of every registration method that has it: a class names its family in ``_family`` ("rgc_gicp", "rgc_gicpst", "rgc_gicpmp",
"rgc_ndt") and takes the parts it has with ``@lsq_seam(...)``.  Each part is bound to the family of the class it was installed on, so a
derived class's object can still be driven through a base class's calls (``FastGICP.linearize(single_thread_object, T)`` is rgc_gicp_linearize)."""
import ctypes as C

import numpy as np

_dp, _fp = C.POINTER(C.c_double), C.POINTER(C.c_float)


def _linearize(family):
    def linearize(self, T, want_H=True):
        """returns (cost, H, b) -- H and b None unless want_H"""
        T = np.ascontiguousarray(T, dtype=np.float64).reshape(16)
        H, b, cost = np.zeros(36), np.zeros(6), C.c_double(0.0)
        self._chk(getattr(self._L, family + "_linearize")(self._h, T.ctypes.data_as(_dp), H.ctypes.data_as(_dp) if want_H else None,
                                                          b.ctypes.data_as(_dp) if want_H else None, C.byref(cost)))
        return (cost.value, H.reshape(6, 6), b) if want_H else (cost.value, None, None)
    return linearize


def _compute_error(family):
    def compute_error(self, T) -> float:
        T = np.ascontiguousarray(T, dtype=np.float64).reshape(16)
        cost = C.c_double(0.0)
        self._chk(getattr(self._L, family + "_compute_error")(self._h, T.ctypes.data_as(_dp), C.byref(cost)))
        return cost.value
    return compute_error


def _num_correspondences(family):
    def num_correspondences(self) -> int:
        n = C.c_int(0)
        self._chk(getattr(self._L, family + "_num_correspondences")(self._h, C.byref(n)))
        return n.value
    return property(num_correspondences)


def _align(family):
    def align(self, guess=None, want_output=True, want_fitness=False):
        """pcl::Registration::align(output, guess): the transformed source cloud (n, 3) float32, or None if want_output=False"""
        g = np.ascontiguousarray(np.eye(4) if guess is None else guess, dtype=np.float32).reshape(16)
        fin, H = np.empty(16, np.float32), np.empty(36)
        fit = C.c_double(0.0)
        it, cv, lf = C.c_int(0), C.c_int(0), C.c_int(0)
        self._chk(getattr(self._L, family + "_align")(self._h, g.ctypes.data_as(_fp), fin.ctypes.data_as(_fp), H.ctypes.data_as(_dp),
                                                      C.byref(fit) if want_fitness else None, C.byref(it), C.byref(cv), C.byref(lf)))
        self._final, self._H = fin.reshape(4, 4), H.reshape(6, 6)
        self._iterations, self._converged, self._lm_failed = it.value, bool(cv.value), bool(lf.value)
        self._fitness = fit.value if want_fitness else None
        if not want_output:
            return None
        out = np.empty((self._n_src, 3), np.float32)
        self._chk(self._L.rgc_get_aligned(self._h, fin.ctypes.data_as(_fp), out.ctypes.data_as(_fp), 12))
        return out
    return align


_PARTS = dict(linearize=_linearize, compute_error=_compute_error, num_correspondences=_num_correspondences, align=_align)


def lsq_seam(*parts):
    """class decorator: install the named parts, over the entry points of the class's ``_family``"""
    def install(cls):
        for name in parts:
            setattr(cls, name, _PARTS[name](cls._family))
        return cls
    return install
